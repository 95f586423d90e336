"""Inputs of the batched small-shape SGPR tests (tests/test_sgpr_batch_gpu.py): the twelve cases and
their generator. Data are drawn as tests/test_sgpr_gpu.py::build draws them (uniform X in [0, 10]^D,
Y = sin(x_0) + 0.3 cos(2 x_last) + 0.05 noise, Z a linspace grid or uniform rows); "days" is the
reference's unnormalised layout, X = arange(89), Z = X[:20]. No GPU is needed to build them.

cond(Kmm) measured with the CPU restatement is 1 ... 8.7e3 ("ragged" is the largest); the cap below
is asserted by the tests, so an ill-conditioned input cannot pass as a well-conditioned one. Not
used on purpose: (65, 20, 1, rq, rand) has cond 8e6, and the days layout with lengthscale 5 and
noise 1e-4 has cond 1e7 (the restatement's own two routes differ by 1e-7 there)."""
import numpy as np

# name: n, M, D, family, Z layout, lengthscale (None: the family's default), noise variance, seed
CASES = {
    "ref":    (113, 10, 1, "se", "grid", None, 1.0, 6),            # the reference's shape
    "m1":     (130, 1, 1, "se", "rand", None, 0.05, 3),            # smallest M
    "m32":    (200, 32, 2, "se*m12", "rand", None, 0.05, 4),       # the M limit; multi-term product
    "ragged": (257, 13, 1, "exp+per+lin", "rand", None, 0.05, 5),  # four chunks + 1 column; Periodic, Linear
    "tiny":   (37, 5, 2, "m32", "rand", None, 0.2, 8),             # N below one chunk
    "n5":     (5, 5, 1, "se", "rand", None, 0.2, 9),               # the monthly series' size; N = M
    "n64":    (64, 20, 1, "m12", "rand", None, 0.05, 10),          # exactly one chunk
    "n65":    (65, 8, 1, "rq", "rand", None, 0.05, 11),            # one chunk + 1; RQ's third parameter
    "d3":     (300, 20, 3, "m52", "rand", None, 0.05, 0),          # several input columns
    "d9":     (100, 8, 9, "se", "rand", 3.0, 0.05, 12),            # the D = 9..16 instance
    "long":   (4096, 20, 1, "se", "grid", 0.5, 0.05, 7),           # the N limit
    "days":   (89, 20, 1, "se", "days", 1.0, 1e-2, 13),            # unnormalised day offsets
}
NAMES = list(CASES)
COND_CAP = 1e5  # cond(Kmm) of every case stays under this (asserted by the tests)


def build(name):
    """(X [n, D], Y [n, 1], Z [M, D], device kernel, oracle kernel, noise variance) of a case."""
    from tests.test_gpu_parity import gpx_kernel, oracle_kernel
    n, M, D, fam, zl, ell, s, seed = CASES[name]
    rng = np.random.default_rng(seed)
    if zl == "days":
        X = np.arange(n, dtype=np.float64)[:, None]
        Y = rng.standard_normal((n, 1))
        Z = X[:M].copy()
    else:
        X = rng.uniform(0, 10, (n, D))
        Y = np.sin(X[:, :1]) + 0.3 * np.cos(2 * X[:, -1:]) + 0.05 * rng.standard_normal((n, 1))
        Z = np.linspace(0, 10, M)[:, None].repeat(D, 1) if zl == "grid" else rng.uniform(0, 10, (M, D))
    gk, ok = gpx_kernel(fam), oracle_kernel(fam)
    if ell is not None:
        gk.lengthscales.assign(ell)
        ok.lengthscales.value = ell
    return X, Y, Z, gk, ok, s
