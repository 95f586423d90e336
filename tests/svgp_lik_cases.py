"""The parity cases of SVGP's per-point route, shared by tests/test_svgp_lik_numpy.py (which checks
on the CPU that the restatement's two routes keep every case inside the caps) and
tests/test_svgp_lik_gpu.py (which compares the device with the restatement). No test here.

The bars are the project's SGPR / VGP rule: 10x the spread between the restatement's two routes —
a property of the references, never of the device result — with floors 1e-12·|F| and
1e-10·(1 + max|g|) per block, capped at 1e-7·|F| and 1e-5·(1 + max|g|) (the ill-conditioned bars
of tests/test_svgp_gpu.py): a case whose bars would exceed the caps is not a usable case.
"""
import functools

import numpy as np

from tests.svgp_lik_numpy import BLOCKS, NumpySVGPLik

# name: N, M, D, family, seed, outliers, df        (scale 0.3 everywhere)
CASES = {
    "tiny":    (5, 3, 1, "se", 0, False, 3.0),             # below a wave and a leaf
    "m1":      (130, 1, 1, "m32", 1, True, 3.0),
    "multi":   (257, 13, 1, "exp+per+lin", 2, True, 4.0),  # k_nn depends on x: the per-row weight shows
    "leaf":    (300, 64, 1, "rq", 3, False, 3.0),          # M exactly one leaf
    "mp128":   (200, 70, 2, "se*m12", 4, True, 5.0),       # Mp = 128
    "node":    (999, 130, 3, "m52", 5, False, 3.0),        # a recursion node
    "chunks":  (2100, 20, 1, "se", 6, True, 3.0),          # two split-K chunks: G_w's chunk sum and padding
    "illcond": (2000, 120, 1, "se", 7, False, 3.0),        # linspace Z, ℓ = 3, num_data = 50000: cond 7e7
}
SCALE = 0.3
CAP_F, CAP_G = 1e-7, 1e-5


def oracle_kernel(fam):
    from tests.test_oracle import oracle_kernel as ok
    return ok(fam)


def build(name):
    """(X, Y, Z, q, R, oracle kernel, num_data, lengthscale override or None) of a case. The data
    are drawn as tests/test_svgp_gpu.py draws them; the outlier cases move 5 % of the rows by about ±2."""
    n, M, D, fam, seed, outliers, _ = CASES[name]
    rng = np.random.default_rng(100 + seed)
    X = rng.uniform(0, 10, (n, D))
    Y = np.sin(X[:, :1]) + 0.3 * np.cos(2 * X[:, -1:]) + 0.05 * rng.standard_normal((n, 1))
    if outliers:
        out = rng.choice(n, max(1, n // 20), replace=False)
        Y[out, 0] += rng.choice([-1.0, 1.0], len(out)) * rng.uniform(1.5, 2.5, len(out))
    grid = name == "illcond"
    Z = np.linspace(0, 10, M)[:, None].repeat(D, 1) if grid else rng.uniform(0, 10, (M, D))
    R = np.tril(rng.standard_normal((M, M)) * 0.05)
    R[np.diag_indices(M)] = rng.uniform(0.3, 1.0, M)
    q = rng.standard_normal(M) * 0.5
    ok = oracle_kernel(fam)
    ell = 3.0 if grid else None
    if ell is not None:
        ok.lengthscales.value = ell
    return X, Y, Z, q, R, ok, (50000 if grid else n), ell


def restatement(name, likelihood="studentt", variance=0.05):
    X, Y, Z, q, R, ok, num_data, _ = build(name)
    om = NumpySVGPLik(ok, Z, likelihood=likelihood, scale=SCALE, variance=variance, df=CASES[name][6],
                      num_data=num_data, q_mu=q, q_sqrt=R)
    return om, X, Y


def bars(om, X, Y):
    """The GPflow-route F and gradient blocks, the bars from the two routes' spread, and the
    row weights g_v."""
    aux = {}
    Fa, ga = om.elbo_and_grads(X, Y, "gpflow", aux=aux)
    Fb, gb = om.elbo_and_grads(X, Y, "w")
    ga = {k: np.atleast_1d(np.asarray(ga[k], dtype=np.float64)) for k in BLOCKS}
    gb = {k: np.atleast_1d(np.asarray(gb[k], dtype=np.float64)) for k in BLOCKS}
    spreadg = {k: float(np.abs(ga[k] - gb[k]).max()) for k in BLOCKS}
    tolF = max(10.0 * abs(Fa - Fb), 1e-12 * abs(Fa))
    tolg = {k: max(10.0 * spreadg[k], 1e-10 * (1.0 + float(np.abs(ga[k]).max()))) for k in BLOCKS}
    return dict(F=Fa, g=ga, tolF=tolF, tolg=tolg, spreadF=abs(Fa - Fb), spreadg=spreadg, g_v=aux["g_v"],
                cond=float(np.linalg.cond(om.kmm())))


@functools.lru_cache(maxsize=None)
def reference(name):
    om, X, Y = restatement(name)
    return bars(om, X, Y)


def assert_inside_caps(name, ref):
    assert ref["tolF"] <= CAP_F * abs(ref["F"]), (name, ref["tolF"], ref["F"])
    for k, t in ref["tolg"].items():
        assert t <= CAP_G * (1.0 + float(np.abs(ref["g"][k]).max())), (name, k, t)
