"""CPU restatement of GPflow 2.9.1 ``models.SVGP`` with a Gaussian or Student-t likelihood — TEST
INFRASTRUCTURE ONLY, in the style of tests/vgp_numpy.py. GPflow's defaults: whitened, full q_sqrt,
zero mean, one latent GP, ``Kmm = k(Z, Z) + 1e-6 I``; minibatch scale ``s = num_data / N``.

With q = q_mu [M], R = tril(q_sqrt), S = R Rᵀ, L = chol(Kmm), φ the likelihood parameter (the
Gaussian variance or the Student-t scale; df is fixed):

    μ_n, v_n  the marginal of q(f) at x_n,   E = Σ_n ve(μ_n, v_n, y_n),   ELBO = s E − KL
    g_μ = s ∂ve/∂μ,   g_v = s ∂ve/∂v,   ∂ELBO/∂φ = s Σ ∂ve/∂φ

ve is GPflow's variational expectation: closed form for the Gaussian, the 20-point Gauss–Hermite
rule ``hermgauss(20)`` for Student-t (tests/vgp_numpy.py states logp).

``route="gpflow"`` is GPflow's: A = L⁻¹ Kmn by triangular solves, v = k_nn − ΣA² + Σ(RᵀA)², and the
gradients as reverse-mode autodiff produces them, through the Cholesky with TensorFlow's rule
(oracle/svgp_oracle.py's elbo_and_grads with per-row g_μ, g_v in place of the Gaussian's).

``route="w"`` forms W = L⁻¹ explicitly, as the device does:

    u = Wᵀq,  P = Wᵀ(S − I)W,  Q = P Kmn,  μ = Kmnᵀu,  v_n = k_nn + Σ_m Kmn[m,n] Q[m,n]
    K̄mn = u g_μᵀ + 2 Q diag(g_v),   â = W Kmn g_μ,   Ĝ_w = W (Kmn diag(g_v) Kmnᵀ) Wᵀ
    ∂q = â − q,   ∂R = tril(2 Ĝ_w R − R + diag(1/R_ii))
    Lᵀ L̄ = −(q âᵀ + 2 (S − I) Ĝ_w),   K̄mm = sym(Wᵀ Φ(Lᵀ L̄) W)
    ∂θ = Σ K̄mn∘∂Kmn + Σ K̄mm∘∂Kmm + Σ_n g_v,n ∂k_nn/∂θ;   ∂Z through ∂k/∂z likewise

The two are equal in exact arithmetic; their difference in floating point measures how far two
correct fp64 implementations may disagree on a case (tests/test_svgp_lik_gpu.py builds its bars
from it). The gradients are pinned by central differences in tests/test_svgp_lik_numpy.py. GPflow
itself is not importable here: parity is against this restatement.
"""
import math

import numpy as np
import scipy.linalg as sla

from oracle.gp_oracle import LOG2PI, OParam
from oracle.svgp_oracle import JITTER, OSVGP, cholesky_grad

GH_X, GH_W = np.polynomial.hermite.hermgauss(20)
GH_W = GH_W / math.sqrt(math.pi)

BLOCKS = ("theta", "lik", "Z", "q_mu", "q_sqrt")


def _tri(L, b, trans=False):
    return sla.solve_triangular(L, b, lower=True, trans=1 if trans else 0, check_finite=False)


class NumpySVGPLik(OSVGP):
    """OSVGP's state and unconstrained-variable plumbing (get_u / set_u / loss_and_grad_u, the
    likelihood parameter in ``self.noise``) with the per-point ELBO of either likelihood."""

    def __init__(self, kernel, Z, likelihood="studentt", scale=1.0, variance=1.0, df=3.0, num_data=None,
                 q_mu=None, q_sqrt=None):
        super().__init__(kernel, Z, num_data=num_data, noise_variance=1.0, q_mu=q_mu, q_sqrt=q_sqrt)
        if likelihood not in ("gaussian", "studentt"):
            raise ValueError(likelihood)
        self.likelihood = likelihood
        self.df = float(df)
        self.noise = (OParam("variance", float(variance), lower=1e-6) if likelihood == "gaussian"
                      else OParam("scale", float(scale)))

    @property
    def lik(self):
        return self.noise

    # ---------------------------------------------------------------- likelihood ------
    def _logp_const(self):
        df = self.df
        return math.lgamma(0.5 * (df + 1)) - math.lgamma(0.5 * df) - 0.5 * (math.log(df) + math.log(math.pi))

    def variational_expectations(self, mu, v, y):
        """(ve [N], ∂ve/∂μ [N], ∂ve/∂v [N], Σ ∂ve/∂φ)."""
        if self.likelihood == "gaussian":
            s = self.noise.value
            qd = (y - mu) ** 2 + v
            return (-0.5 * LOG2PI - 0.5 * math.log(s) - qd / (2 * s), (y - mu) / s, np.full_like(mu, -0.5 / s),
                    float(np.sum(-0.5 / s + qd / (2 * s * s))))
        sc, df = self.noise.value, self.df
        sd = np.sqrt(2.0 * v)
        f = mu[:, None] + sd[:, None] * GH_X[None, :]
        d = y[:, None] - f
        den = sc * sc * df + d * d
        lp = self._logp_const() - math.log(sc) - 0.5 * (df + 1) * np.log1p(d * d / (sc * sc * df))
        dlf = (df + 1) * d / den
        dls = (-1.0 + (df + 1) * d * d / den) / sc
        return lp @ GH_W, dlf @ GH_W, (dlf * GH_X[None, :]) @ GH_W / sd, float(np.sum(dls @ GH_W))

    # ---------------------------------------------------------------- forward ---------
    def kmm(self):
        return self.kernel.K(self.Z) + JITTER * np.eye(len(self.Z))

    def kl(self):
        m, R = self.q_mu, np.tril(self.q_sqrt)
        return 0.5 * (m @ m + np.sum(R * R) - len(m) - np.sum(np.log(np.diag(R) ** 2)))

    def _scale(self, n):
        return 1.0 if self.num_data is None else float(self.num_data) / n

    def elbo(self, X, Y, route="gpflow") -> float:
        return float(self.elbo_and_grads(X, Y, route)[0])

    def training_loss(self, X, Y, route="gpflow") -> float:
        return -self.elbo(X, Y, route)

    # ---------------------------------------------------------------- gradients -------
    def elbo_and_grads(self, X, Y, route="gpflow", aux=None):
        """ELBO and its gradients in constrained space: dict(theta [P], lik (and the same under
        ``noise``), Z [M, D], q_mu [M], q_sqrt [M, M] lower). ``aux``, a dict, receives mu, v, g_mu,
        g_v of the rows."""
        X = np.asarray(X, np.float64).reshape(len(X), -1)
        Y = np.asarray(Y, np.float64).reshape(-1)
        Z, q, R = self.Z, self.q_mu, np.tril(self.q_sqrt)
        M = len(Z)
        s = self._scale(len(X))
        L = np.linalg.cholesky(self.kmm())
        Kmn = self.kernel.K(Z, X)
        kdiag = self.kernel.K_diag(X)
        if route == "gpflow":
            A = _tri(L, Kmn)
            B = R.T @ A
            mu = A.T @ q
            v = kdiag - np.sum(A * A, axis=0) + np.sum(B * B, axis=0)
        elif route == "w":
            W = _tri(L, np.eye(M))
            u = W.T @ q
            Sm1 = R @ R.T - np.eye(M)
            Q = (W.T @ Sm1 @ W) @ Kmn
            mu = Kmn.T @ u
            v = kdiag + np.sum(Kmn * Q, axis=0)
        else:
            raise ValueError(route)
        ve, gmu, gv, gphi = self.variational_expectations(mu, v, Y)
        F = s * float(np.sum(ve)) - self.kl()
        g_mu, g_v = s * gmu, s * gv
        if aux is not None:
            aux.update(mu=mu, v=v, g_mu=g_mu, g_v=g_v)
        if route == "gpflow":
            Abar = np.outer(q, g_mu) + (-2.0 * A + 2.0 * R @ B) * g_v[None, :]
            Rbar = 2.0 * (A * g_v[None, :]) @ B.T - R + np.diag(1.0 / np.diag(R))
            qbar = A @ g_mu - q
            Kmn_bar = _tri(L, Abar, trans=True)
            Kmm_bar = cholesky_grad(L, np.tril(-Kmn_bar @ A.T))
        else:
            Kmn_bar = np.outer(u, g_mu) + 2.0 * Q * g_v[None, :]
            ahat = W @ (Kmn @ g_mu)
            Gh = W @ ((Kmn * g_v[None, :]) @ Kmn.T) @ W.T
            qbar = ahat - q
            Rbar = 2.0 * Gh @ R - R + np.diag(1.0 / np.diag(R))
            Phi = np.tril(-(np.outer(q, ahat) + 2.0 * Sm1 @ Gh))
            Phi[np.diag_indices_from(Phi)] *= 0.5
            Kmm_bar = W.T @ Phi @ W
            Kmm_bar = 0.5 * (Kmm_bar + Kmm_bar.T)
        dKs = self.kernel.dK(np.concatenate([Z, X]))
        dtheta = np.array([np.sum(Kmm_bar * d[:M, :M]) + np.sum(Kmn_bar * d[:M, M:])
                           + np.sum(g_v * np.diag(d)[M:]) for d in dKs])
        dZ = np.einsum("mn,mnd->md", Kmn_bar, self.kernel.dK_dX1(Z, X))
        dZ += 2.0 * np.einsum("mj,mjd->md", Kmm_bar, self.kernel.dK_dX1(Z, Z))
        dlik = s * gphi
        return F, dict(theta=dtheta, lik=dlik, noise=dlik, Z=dZ, q_mu=qbar, q_sqrt=np.tril(Rbar))

    # ---------------------------------------------------------------- prediction ------
    def predict_f(self, Xnew, route="gpflow"):
        """conditional(Xnew, Z, kernel, q_mu, q_sqrt=q_sqrt, white=True), full_cov=False."""
        Xnew = np.asarray(Xnew, np.float64).reshape(len(Xnew), -1)
        R = np.tril(self.q_sqrt)
        L = np.linalg.cholesky(self.kmm())
        Ks = self.kernel.K(self.Z, Xnew)
        As = _tri(L, Ks) if route == "gpflow" else _tri(L, np.eye(len(L))) @ Ks
        RA = R.T @ As
        mean = As.T @ self.q_mu
        var = self.kernel.K_diag(Xnew) - np.sum(As * As, axis=0) + np.sum(RA * RA, axis=0)
        return mean[:, None], var[:, None]

    def predict_y(self, Xnew, route="gpflow"):
        """Gaussian: (mean, var + variance). Student-t: GPflow's quadrature of the conditional mean f
        and of conditional variance + f² = scale² df/(df − 2) + f² over N(mean, var)."""
        mean, var = self.predict_f(Xnew, route)
        if self.likelihood == "gaussian":
            return mean, var + self.noise.value
        cv = self.noise.value ** 2 * self.df / (self.df - 2.0)
        m, v = mean[:, 0], var[:, 0]
        f = m[:, None] + np.sqrt(2.0 * v)[:, None] * GH_X[None, :]
        ey = f @ GH_W
        ey2 = (cv + f * f) @ GH_W
        return ey[:, None], (ey2 - ey * ey)[:, None]
