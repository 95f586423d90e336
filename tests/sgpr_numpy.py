"""CPU restatement of GPflow 2.9.1 ``models.SGPR`` (the collapsed Titsias bound) — TEST
INFRASTRUCTURE ONLY, in the style of tests/svgp_numpy_shard.py. Gaussian likelihood with variance
s = σ², zero mean, one output, ``Kmm = k(Z, Z) + 1e-6 I`` (gpflow.config.default_jitter()).

The bound is evaluated two ways:

``route="gpflow"`` — GPflow's own triangular-solve form (sgpr.py ``elbo`` / ``_common_calculation``):

    L = chol(Kmm);  A = L⁻¹ Kmn / σ;  AAT = A Aᵀ;  B = I + AAT;  LB = chol(B);  c = LB⁻¹ A y / σ
    F = −N/2 log 2π − N/2 log s − Σ log LB_ii − yᵀy/(2s) + cᵀc/2 − Σ k_nn/(2s) + tr(AAT)/2

``route="w"`` — the explicit-inverse form the device computes (gpx_sgpr.hip), W = L⁻¹, WB = LB⁻¹:

    G = Kmn Kmnᵀ,  w = Kmn y,  Ĝ = W G Wᵀ,  â = W w,  B = I + Ĝ/s,  γ = WBᵀ WB â
    F = −N/2 log 2π − N/2 log s − Σ log LB_ii − yᵀy/(2s) + âᵀγ/(2s²) − Σ k_nn/(2s) + tr(Ĝ)/(2s)

The two are equal in exact arithmetic; their difference in floating point measures how far any two
correct fp64 implementations may disagree on a case (tests/test_sgpr_gpu.py sets its tolerances from
it). The gradients follow the same split: route "gpflow" applies L⁻¹ / LB⁻¹ by triangular solves,
route "w" multiplies by the explicit inverses, both from

    H    = (I − B⁻¹)/s − γγᵀ/s³                K̄mn = (Wᵀ H W) Kmn + (Wᵀγ/s²) yᵀ
    K̄mm = Wᵀ [½(I − B⁻¹) − γγᵀ/(2s²) − Ĝ/(2s)] W                  k̄_nn = −1/(2s)
    ∂F/∂s = −N/(2s) + yᵀy/(2s²) − âᵀγ/s³ + Σk_nn/(2s²) − tr(Ĝ)/(2s²) + tr(B⁻¹Ĝ)/(2s²) + γᵀĜγ/(2s⁴)
    ∂F/∂θ = Σ K̄mn∘∂Kmn + Σ K̄mm∘∂Kmm + k̄_nn Σ ∂k_nn;   ∂F/∂Z likewise (K̄mm symmetric: factor 2)

pinned by central finite differences of the GPflow-route F in tests/test_sgpr_oracle.py. GPflow
itself is not importable here: no GPflow-run fixture exists for SGPR, parity is against this
restatement (as for oracle/svgp_oracle.py).
"""
import math

import numpy as np
import scipy.linalg as sla

from oracle.gp_oracle import LOG2PI, OParam

JITTER = 1e-6


def _tri(L, b, trans=False):
    return sla.solve_triangular(L, b, lower=True, trans=1 if trans else 0, check_finite=False)


class NumpySGPR:
    def __init__(self, kernel, X, Y, Z, noise_variance=1.0):
        self.kernel = kernel                  # oracle kernel (K, K_diag, dK, dK_dX1, params)
        self.X = np.asarray(X, np.float64).reshape(len(X), -1)
        self.Y = np.asarray(Y, np.float64).reshape(-1)
        self.Z = np.array(Z, dtype=np.float64).reshape(len(Z), -1)
        self.noise = OParam("variance", float(noise_variance), lower=1e-6)
        self.Z_trainable = True

    # ---------------------------------------------------------------- forward ---------
    def kmm(self):
        return self.kernel.K(self.Z) + JITTER * np.eye(len(self.Z))

    def _common(self, route):
        """Everything both F and the gradients need: Ĝ, â, B⁻¹, γ, Σ log LB_ii and two closures
        applying L⁻¹ · and L⁻ᵀ · by the route's means."""
        s, M = self.noise.value, len(self.Z)
        L = np.linalg.cholesky(self.kmm())
        Kmn = self.kernel.K(self.Z, self.X)
        if route == "gpflow":
            sig = math.sqrt(s)
            A = _tri(L, Kmn) / sig
            AAT = A @ A.T
            Bm = AAT + np.eye(M)
            LB = np.linalg.cholesky(Bm)
            Aerr = A @ self.Y
            c = _tri(LB, Aerr) / sig
            Gh, ah = s * AAT, sig * Aerr
            gam = s * _tri(LB, c, trans=True)              # B⁻¹ â = s LB⁻ᵀ c
            Binv = sla.cho_solve((LB, True), np.eye(M), check_finite=False)
            quad = 0.5 * float(c @ c)                       # = âᵀγ/(2s²)
            trterm = 0.5 * float(np.trace(AAT))             # = tr(Ĝ)/(2s)
            cvec = c
            linv = lambda b: _tri(L, b)                     # noqa: E731
            linvt = lambda b: _tri(L, b, trans=True)        # noqa: E731
        elif route == "w":
            W = _tri(L, np.eye(M))
            G, w = Kmn @ Kmn.T, Kmn @ self.Y
            Gh, ah = W @ G @ W.T, W @ w
            Bm = np.eye(M) + Gh / s
            LB = np.linalg.cholesky(Bm)
            WB = _tri(LB, np.eye(M))
            gam = WB.T @ (WB @ ah)
            Binv = WB.T @ WB
            quad = float(ah @ gam) / (2 * s * s)
            trterm = float(np.trace(Gh)) / (2 * s)
            cvec = WB @ ah / s
            linv = lambda b: W @ b                          # noqa: E731
            linvt = lambda b: W.T @ b                       # noqa: E731
        else:
            raise ValueError(route)
        n = len(self.Y)
        yy, knn = float(self.Y @ self.Y), float(np.sum(self.kernel.K_diag(self.X)))
        F = (-0.5 * n * LOG2PI - 0.5 * n * math.log(s) - float(np.sum(np.log(np.diag(LB))))
             - 0.5 * yy / s + quad - 0.5 * knn / s + trterm)
        return dict(F=F, L=L, LB=LB, Kmn=Kmn, Gh=Gh, ah=ah, gam=gam, Binv=Binv, yy=yy, knn=knn, c=cvec,
                    linv=linv, linvt=linvt)

    def elbo(self, route="gpflow") -> float:
        return float(self._common(route)["F"])

    def training_loss(self, route="gpflow") -> float:
        return -self.elbo(route)

    # ---------------------------------------------------------------- gradients -------
    def elbo_and_grads(self, route="gpflow"):
        """F and its gradients in constrained space: dict(theta [P], noise, Z [M, D])."""
        p = self._common(route)
        s, M, n = self.noise.value, len(self.Z), len(self.Y)
        Gh, ah, gam, Binv, Kmn = p["Gh"], p["ah"], p["gam"], p["Binv"], p["Kmn"]
        linv, linvt = p["linv"], p["linvt"]
        I = np.eye(M)
        H = (I - Binv) / s - np.outer(gam, gam) / s ** 3
        mid = 0.5 * (I - Binv) - np.outer(gam, gam) / (2 * s * s) - Gh / (2 * s)
        # Wᵀ H W Kmn and Wᵀ mid W through the route's L⁻¹ / L⁻ᵀ
        Kmn_bar = linvt(H @ linv(Kmn)) + np.outer(linvt(gam) / (s * s), self.Y)
        Kmm_bar = linvt(linvt(mid.T).T)                     # L⁻ᵀ mid L⁻¹
        Kmm_bar = 0.5 * (Kmm_bar + Kmm_bar.T)
        knn_bar = -0.5 / s
        XA = np.concatenate([self.Z, self.X])
        dtheta = np.array([np.sum(Kmm_bar * d[:M, :M]) + np.sum(Kmn_bar * d[:M, M:])
                           + knn_bar * np.sum(np.diag(d)[M:]) for d in self.kernel.dK(XA)])
        dZ = np.einsum("mn,mnd->md", Kmn_bar, self.kernel.dK_dX1(self.Z, self.X))
        dZ += 2.0 * np.einsum("mj,mjd->md", Kmm_bar, self.kernel.dK_dX1(self.Z, self.Z))
        dnoise = (-0.5 * n / s + 0.5 * p["yy"] / s ** 2 - float(ah @ gam) / s ** 3 + 0.5 * p["knn"] / s ** 2
                  - 0.5 * np.trace(Gh) / s ** 2 + 0.5 * np.sum(Binv * Gh) / s ** 2
                  + 0.5 * float(gam @ Gh @ gam) / s ** 4)
        return p["F"], dict(theta=dtheta, noise=float(dnoise), Z=dZ)

    # ---------------------------------------------------------------- prediction ------
    def predict_f(self, Xnew, route="gpflow"):
        """GPflow's SGPR.predict_f (full_cov=False): mean = Ksᵀ L⁻ᵀ LB⁻ᵀ c,
        var = k** − Σ(L⁻¹Ks)² + Σ(LB⁻¹L⁻¹Ks)²."""
        Xnew = np.asarray(Xnew, np.float64).reshape(len(Xnew), -1)
        p = self._common(route)
        Ks = self.kernel.K(self.Z, Xnew)
        if route == "gpflow":
            t1 = _tri(p["L"], Ks)
            t2 = _tri(p["LB"], t1)
        else:
            M = len(self.Z)
            t1 = _tri(p["L"], np.eye(M)) @ Ks
            t2 = _tri(p["LB"], np.eye(M)) @ t1
        mean = t2.T @ p["c"]
        var = self.kernel.K_diag(Xnew) - np.sum(t1 * t1, axis=0) + np.sum(t2 * t2, axis=0)
        return mean[:, None], var[:, None]

    def predict_y(self, Xnew, route="gpflow"):
        mean, var = self.predict_f(Xnew, route)
        return mean, var + self.noise.value

    # ---------------------------------------------------------------- unconstrained ---
    # tf.Module order on SGPR: inducing_variable.Z < kernel.* < likelihood.variance
    def trainable_params(self):
        return [q for q in self.kernel.params() if q.trainable] + ([self.noise] if self.noise.trainable else [])

    def get_u(self) -> np.ndarray:
        parts = [self.Z.ravel()] if self.Z_trainable else []
        parts.append(np.array([q.u for q in self.trainable_params()]))
        return np.concatenate(parts)

    def set_u(self, u) -> None:
        u = np.asarray(u, dtype=np.float64)
        o = 0
        if self.Z_trainable:
            self.Z = u[o:o + self.Z.size].reshape(self.Z.shape).copy()
            o += self.Z.size
        for q in self.trainable_params():
            q.set_u(float(u[o]))
            o += 1

    def loss_and_grad_u(self, route="gpflow"):
        """(training_loss, ∂loss/∂u) in the flattened trainable-variable order."""
        F, g = self.elbo_and_grads(route)
        parts = [-g["Z"].ravel()] if self.Z_trainable else []
        gt = [-g["theta"][i] * q.dtheta_du() for i, q in enumerate(self.kernel.params()) if q.trainable]
        if self.noise.trainable:
            gt.append(-g["noise"] * self.noise.dtheta_du())
        parts.append(np.array(gt))
        return -float(F), np.concatenate(parts)
