"""CPU restatement of GPflow 2.9.1 ``models.VGP`` — TEST INFRASTRUCTURE ONLY, in the style of
tests/sgpr_numpy.py. GPflow's defaults: whitened, full q_sqrt, zero mean, one output,
``K̃ = k(X, X) + 1e-6 I`` (gpflow.config.default_jitter()); the likelihood is Gaussian (variance s)
or Student-t (scale, fixed df).

With q = q_mu [N], R = tril(q_sqrt) [N, N], L = chol(K̃):

    μ = L q,   A = L R,   v_n = Σ_j A_nj²
    E = Σ_n ve(μ_n, v_n, y_n),   KL = ½(qᵀq + ‖R‖²_F − N − Σ log R_ii²),   ELBO = E − KL

ve is GPflow's variational expectation: for the Gaussian −½ log(2πs) − ((y−μ)² + v)/(2s); for
Student-t the 20-point Gauss–Hermite rule Σ_i (w_i/√π) logp(μ + √(2v) x_i) with

    logp(f) = lgamma((df+1)/2) − lgamma(df/2) − ½(log df + log π) − log scale
              − ½(df+1) log(1 + ((y−f)/scale)²/df)

The gradients, with g_μ = ∂E/∂μ, g_v = ∂E/∂v, C = Lᵀ(g_v ∘ A), t = Lᵀ g_μ:

    ∂q = t − q,   ∂R = tril(2C − R + diag(1/R_ii)),   Lᵀ L̄ = t qᵀ + 2 C Rᵀ
    K̄ = sym(L⁻ᵀ Φ(Lᵀ L̄) L⁻¹)  (Φ: tril with the diagonal halved),   ∂θ = Σ K̄ ∘ ∂K̃/∂θ

``route="gpflow"`` takes L from np.linalg.cholesky and applies L⁻¹ / L⁻ᵀ by triangular solves (the
Cholesky reverse-mode rule as TensorFlow evaluates it). ``route="w"`` forms W = L⁻¹ explicitly,
takes L the way the device does, L = tril(K̃ Wᵀ), and K̄ = sym(Wᵀ Φ W). The two are equal in exact
arithmetic; their difference in floating point measures how far two correct fp64 implementations
may disagree on a case (tests/test_vgp_gpu.py sets its tolerances from it). The gradients are pinned
by central finite differences in tests/test_vgp_oracle.py. GPflow itself is not importable here:
parity is against this restatement.
"""
import math

import numpy as np
import scipy.linalg as sla

from oracle.gp_oracle import LOG2PI, OParam

JITTER = 1e-6
GH_X, GH_W = np.polynomial.hermite.hermgauss(20)
GH_W = GH_W / math.sqrt(math.pi)


def _tri(L, b, trans=False):
    return sla.solve_triangular(L, b, lower=True, trans=1 if trans else 0, check_finite=False)


def gauss_hermite(fun, mu, v):
    """GPflow's ndiagquad: Σ_i (w_i/√π) fun(μ + √(2v) x_i), elementwise over μ, v."""
    f = mu[:, None] + np.sqrt(2.0 * v)[:, None] * GH_X[None, :]
    return fun(f) @ GH_W


class NumpyVGP:
    def __init__(self, kernel, X, Y, likelihood="studentt", scale=1.0, variance=1.0, df=3.0):
        self.kernel = kernel                  # oracle kernel (K, K_diag, dK, params)
        self.X = np.asarray(X, np.float64).reshape(len(X), -1)
        self.Y = np.asarray(Y, np.float64).reshape(-1)
        if likelihood not in ("gaussian", "studentt"):
            raise ValueError(likelihood)
        self.likelihood = likelihood
        self.df = float(df)
        self.lik = (OParam("variance", float(variance), lower=1e-6) if likelihood == "gaussian"
                    else OParam("scale", float(scale)))
        n = len(self.Y)
        self.q = np.zeros(n)
        self.R = np.eye(n)

    # ---------------------------------------------------------------- likelihood ------
    def _logp_const(self):
        df = self.df
        return math.lgamma(0.5 * (df + 1)) - math.lgamma(0.5 * df) - 0.5 * (math.log(df) + math.log(math.pi))

    def logp(self, f, y):
        """log p(y | f), broadcasting."""
        if self.likelihood == "gaussian":
            s = self.lik.value
            return -0.5 * LOG2PI - 0.5 * math.log(s) - 0.5 * (y - f) ** 2 / s
        sc, df = self.lik.value, self.df
        return self._logp_const() - math.log(sc) - 0.5 * (df + 1) * np.log1p(((y - f) / sc) ** 2 / df)

    def variational_expectations(self, mu, v):
        """(ve [N], ∂ve/∂μ [N], ∂ve/∂v [N], Σ ∂ve/∂φ)."""
        y = self.Y
        if self.likelihood == "gaussian":
            s = self.lik.value
            qd = (y - mu) ** 2 + v
            return (-0.5 * LOG2PI - 0.5 * math.log(s) - qd / (2 * s), (y - mu) / s, np.full_like(mu, -0.5 / s),
                    float(np.sum(-0.5 / s + qd / (2 * s * s))))
        sc, df = self.lik.value, self.df
        sd = np.sqrt(2.0 * v)
        f = mu[:, None] + sd[:, None] * GH_X[None, :]
        d = y[:, None] - f
        den = sc * sc * df + d * d
        lp = self._logp_const() - math.log(sc) - 0.5 * (df + 1) * np.log1p(d * d / (sc * sc * df))
        dlf = (df + 1) * d / den
        dls = (-1.0 + (df + 1) * d * d / den) / sc
        return lp @ GH_W, dlf @ GH_W, (dlf * GH_X[None, :]) @ GH_W / sd, float(np.sum(dls @ GH_W))

    # ---------------------------------------------------------------- forward ---------
    def kxx(self):
        return self.kernel.K(self.X) + JITTER * np.eye(len(self.Y))

    def _factor(self, route):
        """L, and two closures applying L⁻¹ · and L⁻ᵀ · by the route's means."""
        Kt = self.kxx()
        L = np.linalg.cholesky(Kt)
        if route == "gpflow":
            return L, (lambda b: _tri(L, b)), (lambda b: _tri(L, b, trans=True))
        if route == "w":
            W = _tri(L, np.eye(len(L)))
            return np.tril(Kt @ W.T), (lambda b: W @ b), (lambda b: W.T @ b)
        raise ValueError(route)

    def kl(self):
        n = len(self.q)
        R = np.tril(self.R)
        return 0.5 * (float(self.q @ self.q) + float(np.sum(R * R)) - n - float(np.sum(np.log(np.diag(R) ** 2))))

    def moments(self, route="gpflow"):
        """(μ, v) of q(f) at the training inputs."""
        L, _, _ = self._factor(route)
        A = L @ np.tril(self.R)
        return L @ self.q, np.sum(A * A, axis=1)

    def elbo(self, route="gpflow") -> float:
        mu, v = self.moments(route)
        return float(np.sum(self.variational_expectations(mu, v)[0])) - self.kl()

    def training_loss(self, route="gpflow") -> float:
        return -self.elbo(route)

    # ---------------------------------------------------------------- gradients -------
    def elbo_and_grads(self, route="gpflow"):
        """ELBO and its gradients in constrained space: dict(theta [P], lik, q_mu [N],
        q_sqrt [N, N] lower triangle)."""
        L, linv, linvt = self._factor(route)
        q, R = self.q, np.tril(self.R)
        A = L @ R
        mu, v = L @ q, np.sum(A * A, axis=1)
        ve, gmu, gv, gphi = self.variational_expectations(mu, v)
        F = float(np.sum(ve)) - self.kl()
        C = L.T @ (gv[:, None] * A)
        t = L.T @ gmu
        dq = t - q
        dR = np.tril(2.0 * C - R + np.diag(1.0 / np.diag(R)))
        P = np.tril(np.outer(t, q) + 2.0 * C @ R.T)
        P[np.diag_indices_from(P)] *= 0.5
        Kbar = linvt(linvt(P.T).T)                          # L⁻ᵀ Φ L⁻¹
        Kbar = 0.5 * (Kbar + Kbar.T)
        dtheta = np.array([np.sum(Kbar * d) for d in self.kernel.dK(self.X)])
        return F, dict(theta=dtheta, lik=float(gphi), q_mu=dq, q_sqrt=dR)

    # ---------------------------------------------------------------- prediction ------
    def predict_f(self, Xnew, route="gpflow"):
        """GPflow's conditional(Xnew, X, kernel, q_mu, q_sqrt=q_sqrt, white=True), full_cov=False:
        A* = L⁻¹ k(X, X*) (no jitter on the cross term), mean = A*ᵀ q, var = k** − ΣA*² + Σ(RᵀA*)²."""
        Xnew = np.asarray(Xnew, np.float64).reshape(len(Xnew), -1)
        _, linv, _ = self._factor(route)
        As = linv(self.kernel.K(self.X, Xnew))
        RA = np.tril(self.R).T @ As
        mean = As.T @ self.q
        var = self.kernel.K_diag(Xnew) - np.sum(As * As, axis=0) + np.sum(RA * RA, axis=0)
        return mean[:, None], var[:, None]

    def predict_y(self, Xnew, route="gpflow"):
        """Gaussian: (mean, var + s). Student-t: GPflow's quadrature of the conditional mean f and of
        conditional variance + f² = scale² df/(df − 2) + f² over N(mean, var)."""
        mean, var = self.predict_f(Xnew, route)
        if self.likelihood == "gaussian":
            return mean, var + self.lik.value
        cv = self.lik.value ** 2 * self.df / (self.df - 2.0)
        m, v = mean[:, 0], var[:, 0]
        ey = gauss_hermite(lambda f: f, m, v)
        ey2 = gauss_hermite(lambda f: cv + f * f, m, v)
        return ey[:, None], (ey2 - ey * ey)[:, None]
