"""CPU reference for ARD (vector-lengthscale) GPR — a helper, not a test.

Values (logML, predictions) come from the committed oracle exactly: an ARD kernel on X is the
isotropic kernel with ℓ = 1 on the pre-scaled inputs X / ℓvec (the same quotients, and /1.0 is
exact), so ``oracle_model`` builds ``O.OGPR`` on the scaled columns (for products: each term's
columns over that term's ℓ, side by side). The oracle has no ∂/∂ℓ_d, so gradients come from a
torch-fp64 autograd restatement of the same arithmetic through ``torch.linalg.cholesky``
(``TorchARD``), itself validated against central differences on u (tests/test_ard_api.py).

A case is a dict: terms = [(family, dim_start, dim_count, ell, variance, alpha)], with ``ell`` a
float (isotropic) or a sequence (ARD); several terms multiply (the reference's Multi-Input
composite). The flat order of the unconstrained variables is the package's: per term
[alpha,] ℓ_0 … ℓ_{dn−1}, variance; then the noise variance when it is trainable.
"""
import math

import numpy as np
import torch

from oracle import gp_oracle as O

LOG2PI = math.log(2.0 * math.pi)
NOISE_LOWER = 1e-6


def make_data(n, D, seed):
    """z-scored random columns; y depends on columns 0 and 1 (when present) only."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, D))
    if n > 1:
        X = (X - X.mean(0)) / X.std(0)
    y = np.sin(1.3 * X[:, 0]) + (0.6 * X[:, 1] if D > 1 else 0.0) + 0.1 * rng.standard_normal(n)
    return X, y[:, None]


def spread(dn, lo=0.5, hi=3.0):
    """unequal lengthscales over [lo, hi]"""
    return [float(v) for v in np.linspace(lo, hi, dn)] if dn > 1 else [0.5 * (lo + hi)]


def case(terms, n, D, noise, seed=0):
    return dict(terms=terms, n=n, D=D, noise=noise, seed=seed)


def single(family, n, D, noise, seed=0, start=0, count=None, variance=1.3, alpha=1.7, ell=None):
    count = D - start if count is None else count
    return case([(family, start, count, spread(count) if ell is None else ell, variance, alpha)], n, D, noise, seed)


def composite(n, D, noise, seed=0):
    """Exponential(ARD over dims 0..D-2) * Exponential(dim D-1): BASELINE config C4's kernel."""
    return case([("exp", 0, D - 1, spread(D - 1), 1.2, None), ("exp", D - 1, 1, 1.5, 0.8, None)], n, D, noise, seed)


def case_id(c):
    t = "*".join(f"{f}{'ard' if not np.isscalar(e) else ''}[{s}:{s + k}]" for f, s, k, e, _, _ in c["terms"])
    return f"{t}-N{c['n']}-D{c['D']}"


# ---------------------------------------------------------------------------------------------
# the package's kernel and model for a case
# ---------------------------------------------------------------------------------------------
def gpx_kernel(c):
    import portfoliooptgp_amd as gpx
    K = gpx.kernels
    cls = {"se": K.SquaredExponential, "m12": K.Matern12, "m32": K.Matern32, "m52": K.Matern52,
           "exp": K.Exponential, "rq": K.RationalQuadratic}
    ks = []
    for fam, s, k, ell, var, alpha in c["terms"]:
        kw = dict(variance=var, lengthscales=ell, active_dims=list(range(s, s + k)))
        if fam == "rq":
            kw["alpha"] = alpha
        ks.append(cls[fam](**kw))
    return ks[0] if len(ks) == 1 else K.Product(ks)


def gpx_model(c, trainable_noise=True):
    import portfoliooptgp_amd as gpx
    X, Y = make_data(c["n"], c["D"], c["seed"])
    m = gpx.models.GPR((X, Y), kernel=gpx_kernel(c), noise_variance=c["noise"])
    if not trainable_noise:
        gpx.set_trainable(m.likelihood.variance, False)
    return m


# ---------------------------------------------------------------------------------------------
# values: the oracle on pre-scaled inputs
# ---------------------------------------------------------------------------------------------
def scale_inputs(c, X):
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    cols = []
    for _, s, k, ell, _, _ in c["terms"]:
        ellv = np.full(k, ell) if np.isscalar(ell) else np.asarray(ell, dtype=np.float64)
        cols.append(X[:, s:s + k] / ellv)
    return np.hstack(cols)


def oracle_model(c):
    cls = {"se": O.OSquaredExponential, "m12": O.OMatern12, "m32": O.OMatern32, "m52": O.OMatern52,
           "exp": O.OExponential, "rq": O.ORationalQuadratic}
    X, Y = make_data(c["n"], c["D"], c["seed"])
    ks, o = [], 0
    for fam, _, k, _, var, alpha in c["terms"]:
        kw = dict(variance=var, lengthscales=1.0, active_dims=list(range(o, o + k)))
        if fam == "rq":
            kw["alpha"] = alpha
        ks.append(cls[fam](**kw))
        o += k
    kern = ks[0] if len(ks) == 1 else O.OProduct(ks)
    return O.OGPR(scale_inputs(c, X), Y, kern, noise_variance=c["noise"])


def oracle_values(c, xnews):
    """dict: loss, cond, and per xnew (fmean, fvar, fcov) from the oracle on scaled inputs"""
    om = oracle_model(c)
    out = dict(loss=-om.log_marginal_likelihood(), cond=float(np.linalg.cond(om._Ky())), pred=[])
    for xn in xnews:
        xs = scale_inputs(c, xn)
        fm, fv = om.predict_f(xs)
        _, fc = om.predict_f(xs, full_cov=True)
        out["pred"].append((fm, fv, fc))
    return out


# ---------------------------------------------------------------------------------------------
# gradients: torch-fp64 autograd restatement
# ---------------------------------------------------------------------------------------------
def _softplus_inv(t):
    return O.softplus_inverse(t)


class TorchARD:
    """−logML(u) of a case with the package's arithmetic (a = x/ℓ_d, the expanded square distance,
    the 1e-36 clamp of the K_r kinds, θ = lower + softplus(u)) in torch fp64."""

    def __init__(self, c, trainable_noise=True, data=None):
        self.c = c
        X, Y = make_data(c["n"], c["D"], c["seed"]) if data is None else data
        self.X = torch.as_tensor(np.asarray(X, dtype=np.float64))
        self.y = torch.as_tensor(np.asarray(Y, dtype=np.float64).reshape(-1))
        self.trainable_noise = trainable_noise
        u, self.layout = [], []   # layout: per term (family, start, count, i_alpha, i_ell0, n_ell, i_var)
        for fam, s, k, ell, var, alpha in c["terms"]:
            ia = None
            if fam == "rq":
                ia = len(u)
                u.append(_softplus_inv(alpha))
            ie = len(u)
            ells = [ell] if np.isscalar(ell) else list(ell)
            u.extend(_softplus_inv(float(e)) for e in ells)
            iv = len(u)
            u.append(_softplus_inv(var))
            self.layout.append((fam, s, k, ia, ie, len(ells), iv))
        self.n_kernel = len(u)
        self.noise_u = _softplus_inv(c["noise"] - NOISE_LOWER)
        if trainable_noise:
            u.append(self.noise_u)
        self.u0 = np.asarray(u, dtype=np.float64)

    def K(self, th, X, X2=None):
        X2 = X if X2 is None else X2
        out = None
        for fam, s, k, ia, ie, ne, iv in self.layout:
            ell = th[ie:ie + ne]          # (one entry broadcasts: the isotropic term)
            a, b = X[:, s:s + k] / ell, X2[:, s:s + k] / ell
            # sums over d in order, each product rounded on its own (so r² is exactly 0 on the diagonal)
            dot, sa, sb = a[:, :1] * b[:, :1].T, a[:, 0] * a[:, 0], b[:, 0] * b[:, 0]
            for d in range(1, k):
                dot = dot + a[:, d:d + 1] * b[:, d:d + 1].T
                sa = sa + a[:, d] * a[:, d]
                sb = sb + b[:, d] * b[:, d]
            r2 = -2.0 * dot + (sa[:, None] + sb[None, :])
            if fam == "se":
                g = torch.exp(-0.5 * r2)
            elif fam == "rq":
                g = (1.0 + 0.5 * r2 / th[ia]) ** (-th[ia])
            else:
                r = torch.sqrt(torch.clamp(r2, min=1e-36))
                if fam == "m12":
                    g = torch.exp(-r)
                elif fam == "exp":
                    g = torch.exp(-0.5 * r)
                elif fam == "m32":
                    g = (1.0 + math.sqrt(3.0) * r) * torch.exp(-math.sqrt(3.0) * r)
                else:
                    g = (1.0 + math.sqrt(5.0) * r + 5.0 / 3.0 * r2.clamp(min=1e-36)) * torch.exp(-math.sqrt(5.0) * r)
            kt = th[iv] * g
            out = kt if out is None else out * kt
        return out

    def theta(self, u):
        th = torch.nn.functional.softplus(u[:self.n_kernel])
        un = u[self.n_kernel] if self.trainable_noise else torch.tensor(self.noise_u, dtype=torch.float64)
        return th, NOISE_LOWER + torch.nn.functional.softplus(un)

    def loss_t(self, u):
        th, noise = self.theta(u)
        n = self.X.shape[0]
        Ky = self.K(th, self.X) + noise * torch.eye(n, dtype=torch.float64)
        L = torch.linalg.cholesky(Ky)
        z = torch.linalg.solve_triangular(L, self.y[:, None], upper=False)
        return 0.5 * (z * z).sum() + torch.log(torch.diagonal(L)).sum() + 0.5 * n * LOG2PI

    def loss(self, u):
        with torch.no_grad():
            return float(self.loss_t(torch.as_tensor(np.asarray(u, dtype=np.float64))))

    def loss_and_grad(self, u=None):
        ut = torch.tensor(self.u0 if u is None else np.asarray(u, dtype=np.float64), requires_grad=True)
        f = self.loss_t(ut)
        f.backward()
        return float(f.detach()), ut.grad.numpy().copy()

    def central_differences(self, u=None, h=1e-5):
        u = (self.u0 if u is None else np.asarray(u, dtype=np.float64)).copy()
        g = np.empty_like(u)
        for k in range(len(u)):
            up, um = u.copy(), u.copy()
            up[k] += h
            um[k] -= h
            g[k] = (self.loss(up) - self.loss(um)) / (2.0 * h)
        return g


# ---------------------------------------------------------------------------------------------
# the cases of tests/test_ard_gpu.py (each validated on the CPU by tests/test_ard_api.py:
# autograd against central differences within 1e-5 relative)
# ---------------------------------------------------------------------------------------------
PARITY_CASES = [
    single("se", 5, 2, 1e-2, seed=1),
    single("se", 60, 3, 1e-2, seed=2),
    single("se", 67, 13, 1e-2, seed=3, ell=spread(13, 2.0, 6.0)),   # fills the θ row
    single("se", 200, 5, 1e-2, seed=4, ell=spread(5, 1.0, 3.0)),
    single("se", 600, 3, 1e-2, seed=5),
    single("se", 200, 4, 1e-2, seed=6, start=1, count=3),           # dim_start > 0
    single("m12", 67, 2, 1e-3, seed=7),
    single("m32", 200, 3, 1e-3, seed=8),
    single("m52", 60, 2, 1e-2, seed=9),
    single("m52", 600, 5, 1e-2, seed=10, ell=spread(5, 1.0, 3.0)),
    single("exp", 200, 2, 1e-3, seed=11),
    single("rq", 67, 3, 1e-2, seed=12),
    single("rq", 600, 2, 1e-2, seed=13),
    composite(5, 3, 1e-2, seed=14),
    composite(67, 5, 1e-3, seed=15),
    composite(200, 5, 1e-2, seed=16),
    composite(600, 5, 1e-2, seed=17),
]


def relevance_data(n=120, seed=21):
    """D = 3, y a function of columns 0 and 1 only (the end-to-end fit's data)."""
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((n, 3))
    X = (X - X.mean(0)) / X.std(0)
    y = np.sin(1.5 * X[:, 0]) + 0.8 * np.cos(1.1 * X[:, 1]) + 0.05 * rng.standard_normal(n)
    return X, y[:, None]
