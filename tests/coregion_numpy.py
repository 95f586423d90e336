"""CPU reference for GPR with a Coregion kernel — a helper, not a test.

gpflow.kernels.Coregion (2.9.1), restated: parameters ``W`` [P, R] (identity transform, default
0.1·ones, any sign) and ``kappa`` [P] (softplus, default ones), tf.Module order W, kappa;
``B = W Wᵀ + diag(κ)``; ``K(X, X2)[i, j] = B[a_i, b_j]`` with a / b the one active column cast to
int; ``K_diag(X)[i] = B[a_i, a_i]``. In a product every other factor multiplies elementwise. The
model's one Gaussian noise σn² is shared by all outputs (predict_y adds it; κ is not noise).

Values (logML, predict_f, predict_y, full_cov, cond) come from the committed oracle's own GPR
(``O.OGPR``) and its kernels for the partner terms — ARD partners through pre-scaled inputs exactly
as tests/ard_numpy.py does — with ``OCoregion`` below as one more factor of ``O.OProduct``.
Gradients come from a torch-fp64 autograd restatement (``TorchCoregion``: W identity, κ and the
partners softplus, noise trainable or frozen; the partners' arithmetic is ``ard_numpy.TorchARD.K``),
validated against central differences in tests/test_coregion_api.py.

A case is a dict: partners = [(family, dim_start, dim_count, ell, variance, alpha)] (may be empty:
Coregion alone), P, R, W, kappa, n, Df (feature columns; the index column is column Df), noise,
seed, layout (how the rows' asset indices are laid out), first (the Coregion term is the product's
first factor instead of its last). The flat order of the unconstrained variables is the package's:
the terms in product order — a partner [alpha,] ℓ.., variance; Coregion W row-major then κ — then
the noise variance when it is trainable.
"""
import numpy as np
import torch

from oracle import gp_oracle as O
from tests import ard_numpy as A

NOISE_LOWER = A.NOISE_LOWER
LOG2PI = A.LOG2PI


# ---------------------------------------------------------------------------------------------
# data: feature columns + the asset index column
# ---------------------------------------------------------------------------------------------
def index_layout(n, P, layout, rng):
    """the n rows' asset indices. sorted: asset by asset, near-equal counts; robin: 0,1,..,P-1,0,..;
    perm: a random permutation of robin; ragged: unequal counts with asset P-1 holding one row,
    asset by asset; empty: as sorted over P-1 assets — asset P-1 has no rows."""
    if layout == "robin":
        return np.arange(n) % P
    if layout == "perm":
        return rng.permutation(np.arange(n) % P)
    if layout == "empty":
        return np.sort(np.arange(n) % (P - 1))
    if layout == "ragged":
        if P == 1 or n < P:
            return np.sort(np.arange(n) % P)
        w = np.arange(P - 1, 0, -1, dtype=np.float64)  # decreasing counts over assets 0..P-2
        cnt = np.maximum(1, np.floor((n - 1) * w / w.sum()).astype(int))
        cnt[0] += (n - 1) - cnt.sum()
        return np.concatenate([np.full(c, p) for p, c in enumerate(cnt)] + [np.array([P - 1])])
    return np.sort(np.arange(n) % P)


def make_data(c):
    """X [n, Df + 1] (z-scored random features, then the asset index) and Y [n, 1]: every asset a
    signed multiple of one smooth function of the features plus an own offset."""
    n, Df, P = c["n"], c["Df"], c["P"]
    rng = np.random.default_rng(c["seed"])
    F = rng.standard_normal((n, max(Df, 1)))
    if n > 1:
        F = (F - F.mean(0)) / F.std(0)
    idx = index_layout(n, P, c["layout"], rng)
    sign = np.where(np.arange(P) % 2 == 0, 1.0, -0.7)
    y = sign[idx] * np.sin(1.3 * F[:, 0]) + 0.2 * np.cos(idx) + 0.1 * rng.standard_normal(n)
    X = np.concatenate([F[:, :Df], idx[:, None].astype(np.float64)], axis=1)
    return X, y[:, None]


def mixed_sign_W(P, R, seed):
    rng = np.random.default_rng(seed)
    W = rng.uniform(0.3, 1.0, size=(P, R))
    W[(np.arange(P)[:, None] + np.arange(R)[None, :]) % 2 == 1] *= -1.0
    return W


def case(partners, P, R, n, Df, noise=1e-2, seed=0, layout="sorted", first=False):
    rng = np.random.default_rng(7000 + seed)
    return dict(partners=partners, P=P, R=R, W=mixed_sign_W(P, R, 9000 + seed),
                kappa=rng.uniform(0.2, 0.8, size=P), n=n, Df=Df, noise=noise, seed=seed, layout=layout, first=first)


def case_id(c):
    t = "*".join(f"{f}{'ard' if not np.isscalar(e) else ''}[{s}:{s + k}]" for f, s, k, e, _, _ in c["partners"])
    cg = f"coreg{c['P']}x{c['R']}"
    return f"{cg + '*' + t if c['first'] else t + '*' + cg}-N{c['n']}-{c['layout']}".replace("**", "*").strip("*")


# ---------------------------------------------------------------------------------------------
# the package's kernel and model for a case
# ---------------------------------------------------------------------------------------------
def gpx_kernel(c):
    import portfoliooptgp_amd as gpx
    K = gpx.kernels
    ks = []
    if c["partners"]:
        pk = A.gpx_kernel(dict(terms=c["partners"]))
        ks = list(pk.kernels) if isinstance(pk, K.Product) else [pk]
    cg = K.Coregion(output_dim=c["P"], rank=c["R"], active_dims=[c["Df"]])
    cg.W.assign(c["W"])
    cg.kappa.assign(c["kappa"])
    ks = [cg] + ks if c["first"] else ks + [cg]
    return ks[0] if len(ks) == 1 else K.Product(ks)


def gpx_model(c, trainable_noise=True, data=None):
    import portfoliooptgp_amd as gpx
    X, Y = make_data(c) if data is None else data
    m = gpx.models.GPR((X, Y), kernel=gpx_kernel(c), noise_variance=c["noise"])
    if not trainable_noise:
        gpx.set_trainable(m.likelihood.variance, False)
    return m


# ---------------------------------------------------------------------------------------------
# values: the oracle's GPR with one more product factor
# ---------------------------------------------------------------------------------------------
def output_covariance(W, kappa):
    W = np.asarray(W, dtype=np.float64)
    return W @ W.T + np.diag(np.asarray(kappa, dtype=np.float64))


class OCoregion(O.OKernel):
    """gpflow.kernels.Coregion as an oracle kernel on column ``col``. Values only (the oracle's
    parameter list is for positive parameters; the gradients are TorchCoregion's)."""

    def __init__(self, W, kappa, col):
        self.W, self.kappa, self.col = np.asarray(W, dtype=np.float64), np.asarray(kappa, dtype=np.float64), col
        self._kp = [O.OParam(f"kappa[{p}]", float(v)) for p, v in enumerate(self.kappa)]

    def params(self):
        return list(self._kp)

    def _idx(self, X):
        return np.asarray(X, dtype=np.float64).reshape(len(X), -1)[:, self.col].astype(np.int64)

    def K(self, X, X2=None):
        B = output_covariance(self.W, self.kappa)
        a = self._idx(X)
        b = a if X2 is None else self._idx(X2)
        return B[a][:, b]

    def K_diag(self, X):
        a = self._idx(X)
        return np.diag(output_covariance(self.W, self.kappa))[a]


def _scaled(c, X):
    """the partners' columns over their ℓ side by side (ard_numpy.scale_inputs), then the index column"""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    cols = [A.scale_inputs(dict(terms=c["partners"]), X)] if c["partners"] else []
    return np.hstack(cols + [X[:, c["Df"]:c["Df"] + 1]])


def oracle_model(c, data=None):
    cls = {"se": O.OSquaredExponential, "m12": O.OMatern12, "m32": O.OMatern32, "m52": O.OMatern52,
           "exp": O.OExponential, "rq": O.ORationalQuadratic}
    X, Y = make_data(c) if data is None else data
    ks, o = [], 0
    for fam, _, k, _, var, alpha in c["partners"]:
        kw = dict(variance=var, lengthscales=1.0, active_dims=list(range(o, o + k)))
        if fam == "rq":
            kw["alpha"] = alpha
        ks.append(cls[fam](**kw))
        o += k
    cg = OCoregion(c["W"], c["kappa"], o)
    ks = [cg] + ks if c["first"] else ks + [cg]
    kern = ks[0] if len(ks) == 1 else O.OProduct(ks)
    return O.OGPR(_scaled(c, X), Y, kern, noise_variance=c["noise"])


def oracle_values(c, xnews, data=None):
    """dict: loss, cond (as ard_numpy.oracle_values computes it), and per xnew (fmean, fvar, fcov)"""
    om = oracle_model(c, data)
    out = dict(loss=-om.log_marginal_likelihood(), cond=float(np.linalg.cond(om._Ky())), pred=[])
    for xn in xnews:
        xs = _scaled(c, xn)
        fm, fv = om.predict_f(xs)
        _, fc = om.predict_f(xs, full_cov=True)
        out["pred"].append((fm, fv, fc))
    return out


def prediction_inputs(c, m, rng):
    """m prediction rows: random features, asset indices cycling over all P assets"""
    F = rng.standard_normal((m, c["Df"]))
    return np.concatenate([F, (np.arange(m) % c["P"])[:, None].astype(np.float64)], axis=1)


# ---------------------------------------------------------------------------------------------
# gradients: torch-fp64 autograd restatement
# ---------------------------------------------------------------------------------------------
class TorchCoregion:
    """−logML(u) of a case in torch fp64: K = Π partners (ard_numpy.TorchARD.K) ∘ B[a, b],
    B = W Wᵀ + diag(κ), W = u_W (identity), κ = softplus(u_κ), partners' θ = softplus(u),
    σn² = 1e-6 + softplus(u_n)."""

    def __init__(self, c, trainable_noise=True, data=None):
        self.c = c
        X, Y = make_data(c) if data is None else data
        self.X = torch.as_tensor(np.asarray(X, dtype=np.float64))
        self.y = torch.as_tensor(np.asarray(Y, dtype=np.float64).reshape(-1))
        self.idx = torch.as_tensor(np.asarray(X)[:, c["Df"]].astype(np.int64))
        self.trainable_noise = trainable_noise
        P, R = c["P"], c["R"]
        self.part = A.TorchARD(dict(terms=c["partners"], n=c["n"], D=c["Df"], noise=c["noise"], seed=c["seed"]),
                               trainable_noise=False, data=(X, Y))
        npk = self.part.n_kernel
        up = self.part.u0[:npk]
        ucg = np.concatenate([np.asarray(c["W"], dtype=np.float64).reshape(-1),
                              [O.softplus_inverse(float(k)) for k in c["kappa"]]])
        self.o_cg, self.o_part = (0, P * R + P) if c["first"] else (npk, 0)
        self.n_kernel = npk + P * R + P
        self.noise_u = O.softplus_inverse(c["noise"] - NOISE_LOWER)
        u = np.concatenate([ucg, up] if c["first"] else [up, ucg])
        self.u0 = np.concatenate([u, [self.noise_u]]) if trainable_noise else u

    def B(self, u):
        P, R = self.c["P"], self.c["R"]
        W = u[self.o_cg:self.o_cg + P * R].reshape(P, R)
        kappa = torch.nn.functional.softplus(u[self.o_cg + P * R:self.o_cg + P * R + P])
        return W @ W.T + torch.diag(kappa)

    def K(self, u, X, idx, X2=None, idx2=None):
        B = self.B(u)
        Kc = B[idx][:, idx if idx2 is None else idx2]
        if self.part.n_kernel == 0:
            return Kc
        th = torch.nn.functional.softplus(u[self.o_part:self.o_part + self.part.n_kernel])
        return self.part.K(th, X, X2) * Kc

    def loss_t(self, u):
        un = u[self.n_kernel] if self.trainable_noise else torch.tensor(self.noise_u, dtype=torch.float64)
        noise = NOISE_LOWER + torch.nn.functional.softplus(un)
        n = self.X.shape[0]
        Ky = self.K(u, self.X, self.idx) + noise * torch.eye(n, dtype=torch.float64)
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

    def output_covariance(self, u):
        with torch.no_grad():
            return self.B(torch.as_tensor(np.asarray(u, dtype=np.float64))).numpy()

    def coregion_slots(self, p):
        """indices into u of asset p's W row and κ entry"""
        P, R = self.c["P"], self.c["R"]
        return list(range(self.o_cg + p * R, self.o_cg + (p + 1) * R)) + [self.o_cg + P * R + p]


# ---------------------------------------------------------------------------------------------
# the cases of tests/test_coregion_gpu.py (each validated on the CPU by tests/test_coregion_api.py).
# Sizes: N = 5 / 60 one 64-tile; 67 Np = 128 (the launch chain, the first off-diagonal tile);
# 200 Np = 256 (the recursion, off-diagonal 64-tiles); 600 the 128-tile instances.
# ---------------------------------------------------------------------------------------------
SE1 = [("se", 0, 1, 1.4, 1.3, None)]
EXP3 = [("exp", 0, 3, 1.8, 1.2, None)]
SE_ARD = [("se", 0, 2, [0.9, 2.1], 1.1, None)]
EXP_EXP = [("exp", 0, 2, 1.6, 1.2, None), ("exp", 2, 1, 1.5, 0.8, None)]

PARITY_CASES = [
    case(SE1, 2, 1, 5, 1, seed=1, layout="sorted"),
    case(EXP3, 3, 1, 60, 3, seed=2, layout="robin"),
    case(SE_ARD, 5, 1, 67, 2, seed=3, layout="perm"),
    case([], 2, 2, 200, 1, seed=4, layout="ragged"),                       # Coregion alone
    case(SE1, 4, 2, 600, 1, seed=5, layout="ragged"),                      # 15 θ values: the row's limit
    case(SE1, 6, 1, 200, 1, seed=6, layout="empty"),                       # 15 θ values; asset 5 has no rows
    case(EXP_EXP, 3, 1, 67, 3, seed=7, layout="sorted"),                   # three factors
    case(EXP3, 5, 1, 600, 3, seed=8, layout="perm"),
    case(SE_ARD, 2, 2, 60, 2, seed=9, layout="robin", first=True),         # Coregion as the first factor
    case([], 3, 1, 5, 1, seed=10, layout="robin"),
    case(EXP3, 4, 2, 200, 3, seed=11, layout="perm"),
]


# ---------------------------------------------------------------------------------------------
# the end-to-end fit's data: three assets drawn from a GP with a known B, one negative off-diagonal
# ---------------------------------------------------------------------------------------------
SIGN_B = np.array([[1.0, 0.8, -0.7], [0.8, 1.0, -0.5], [-0.7, -0.5, 1.0]])


def sign_data(n_per=60, seed=32):
    """3 × n_per rows on a shared time grid t in [0, 6]: f ~ GP(0, SE(ℓ = 1)(t, t') · SIGN_B[a, b]),
    y = f + 0.05·ε. Asset 2 moves against assets 0 and 1."""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 6.0, n_per)
    Kt = np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2)
    Kf = np.kron(SIGN_B, Kt) + 1e-10 * np.eye(3 * n_per)
    f = np.linalg.cholesky(Kf) @ rng.standard_normal(3 * n_per)
    y = f + 0.05 * rng.standard_normal(3 * n_per)
    X = np.stack([np.tile(t, 3), np.repeat(np.arange(3.0), n_per)], axis=1)
    return X, y[:, None]


def sign_case(n_per=60):
    """the fit's start: SE(ℓ = 1, σ² = 1) × Coregion(3, 1) at GPflow's defaults (W = 0.1·ones — every
    off-diagonal of B positive, so the fit has to turn a sign — κ = 1), noise 0.1 trainable"""
    c = case([("se", 0, 1, 1.0, 1.0, None)], 3, 1, 3 * n_per, 1, noise=0.1, seed=0)
    c["W"] = 0.1 * np.ones((3, 1))
    c["kappa"] = np.ones(3)
    return c
