"""Inputs of the batched small-shape SVGP tests (tests/test_svgp_batch_gpu.py): the thirteen cases
(n, M, D, family, layout, noise) and their generators. "rand" is tests/test_svgp_gpu.py::_case
(uniform X and Z in [0, 10]^D, random q_mu, lower q_sqrt with diagonal in [0.3, 1]); "days" is the
reference's layout (test_scripts/GPR.py:118-138): X = arange(n), Z = X[:M], Y z-scored normal draws,
the same q generators. No GPU is needed to build them."""
import numpy as np

CASES = [
    (89, 20, 1, "se", "days", 1e-4),
    (19, 19, 1, "exp+per+lin", "days", 1e-4),
    (5, 5, 1, "se*m12", "days", 1e-4),
    (89, 20, 1, "rq", "days", 1e-4),
    (89, 20, 1, "se+m12", "days", 1e-4),
    (89, 20, 1, "exp+per", "days", 1e-4),
    (300, 20, 1, "m12", "days", 1e-4),
    (130, 1, 1, "m32", "rand", 0.05),
    (257, 32, 2, "se*m12", "rand", 0.05),
    (64, 17, 1, "m12", "rand", 0.05),
    (65, 16, 3, "m52", "rand", 0.05),
    (1000, 31, 1, "exp+per", "rand", 0.05),
    (1, 3, 2, "se+m12", "rand", 0.05),
]
# seeds of the "rand" cases, picked on the CPU so that cond(Kmm + 1e-6 I) stays under the cap (a 1-D random Z
# under exp+per reaches 1e4..2e5 with other seeds; 122 gives 3.7e3)
RAND_SEED = {7: 107, 8: 108, 9: 109, 10: 110, 11: 122, 12: 112}
COND_CAP = 1e4  # cond(Kmm + 1e-6 I) of every case stays under this (asserted by the tests)


def days_xy(n, seed):
    rng = np.random.default_rng(1000 + seed)
    X = np.arange(n, dtype=np.float64)[:, None]
    y = rng.standard_normal(n)
    if n > 1:
        y = (y - y.mean()) / y.std(ddof=1)
    return X, y[:, None]


def make_case(i):
    """dict(X, Y, Z, q, R, gk, ok, noise, n, M, D, fam) of case i; gk / ok are fresh kernels."""
    from tests.test_gpu_parity import gpx_kernel, oracle_kernel
    from tests.test_svgp_gpu import _case
    n, M, D, fam, layout, noise = CASES[i]
    if layout == "rand":
        X, Y, Z, q, R, gk, ok = _case(n, M, D, fam, RAND_SEED[i])
    else:
        X, Y = days_xy(n, i)
        Z = X[:M].copy()
        rng = np.random.default_rng(2000 + i)
        R = np.tril(rng.standard_normal((M, M)) * 0.05)
        R[np.diag_indices(M)] = rng.uniform(0.3, 1.0, M)
        q = rng.standard_normal(M) * 0.5
        gk, ok = gpx_kernel(fam), oracle_kernel(fam)
    return dict(X=X, Y=Y, Z=Z, q=q, R=R, gk=gk, ok=ok, noise=noise, n=n, M=M, D=D, fam=fam)


def cond_kmm(case):
    K = case["ok"].K(case["Z"]) + 1e-6 * np.eye(case["M"])
    return float(np.linalg.cond(K))
