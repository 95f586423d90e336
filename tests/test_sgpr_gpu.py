"""SGPR on the GPU (libgpx.so gpx_sgpr_*) against the CPU restatement (tests/sgpr_numpy.py).

Tolerances are not constants. The collapsed bound cancels Σk_nn/s against tr(Ĝ)/s, so how far two
correct fp64 evaluations may differ depends on the case; per case the restatement is evaluated by
its two routes (GPflow's triangular solves, and the explicit inverses the device uses) and the
spread between them — a property of the references, never of the device result — sets the bar:

    |F_dev − F_gpflow|  <=  max(10 · |F_gpflow − F_w|,          1e-12 · |F|)
    |g_dev − g_gpflow|  <=  max(10 · max|g_gpflow − g_w|,       1e-10 · (1 + max|g|))   per block

(10x: the device sums in another order again — split-K, MFMA accumulation). Every case but the one
marked ill-conditioned must also have cond(Kmm) <= 1e5 and resulting bars <= 1e-8·|F| and
<= 1e-6·(1 + max|g|); both are asserted.

Spreads of the two routes measured on the CPU (relative to |F|; gradient blocks relative to
1 + max|g|), with cond(Kmm):

    case      cond(Kmm)   F         theta     noise     Z
    ref       2.1e1       0         3.8e-15   4.1e-16   5.9e-15
    m1        1.0         0         0         0         1.8e-16
    ragged    8.7e3       1.5e-12   1.7e-10   4.0e-12   1.0e-9
    mp128     3.4e1       6.5e-16   5.2e-16   5.4e-16   7.9e-15
    leaf      3.3e4       5.1e-13   1.5e-12   6.4e-13   4.5e-11
    splitk    3.9e1       2.6e-14   1.0e-13   2.3e-14   1.4e-13
    d3        2.0e1       0         7.9e-16   1.2e-16   2.6e-14
    ill       7.0e7       2.6e-6    1.0e-6    4.0e-7    6.5e-3
    tiny      3.3         0         1.3e-16   2.0e-16   5.9e-16

so the floors (1e-12, 1e-10) are the bar on most well-conditioned cases and the spread on
"ragged", "leaf" and "ill".
"""
import functools

import numpy as np
import pytest
import scipy.optimize

pytestmark = pytest.mark.gpu

import portfoliooptgp_amd as gpx  # noqa: E402
from tests.sgpr_numpy import NumpySGPR  # noqa: E402
from tests.test_gpu_parity import gpx_kernel, oracle_kernel  # noqa: E402

# name: n, M, D, family, Z layout, lengthscale(s) (None: the family's defaults), noise variance, seed
CASES = {
    "ref":    (113, 10, 1, "se", "grid", None, 1.0, 6),          # the reference's shapes
    "m1":     (130, 1, 1, "se", "rand", None, 0.05, 3),          # smallest M
    "ragged": (257, 13, 1, "exp+per+lin", "rand", None, 0.05, 5),  # ragged N, multi-term kernel
    "mp128":  (200, 70, 2, "se*m12", "rand", None, 0.05, 4),     # Mp = 128, crosses a leaf
    "leaf":   (300, 64, 2, "se", "rand", None, 0.05, 2),         # exactly one leaf, no padding
    "splitk": (2100, 20, 1, "se", "grid", 0.5, 0.05, 7),         # two split-K chunks, ragged last one
    "d3":     (1500, 100, 3, "m52", "rand", None, 0.05, 0),      # three input columns, Matern kernel
    "ill":    (2000, 120, 1, "se", "grid", 3.0, 0.01, 1),        # grid Z, long lengthscale: ill-conditioned
    "tiny":   (37, 5, 2, "m32", "rand", None, 0.2, 8),           # N below one 64-column tile
}
WELL = [c for c in CASES if c != "ill"]


def _set_ell(gk, ok, ell):
    gk.lengthscales.assign(ell)
    ok.lengthscales.value = ell


def build(name):
    """(X, Y, Z, device kernel, oracle kernel, noise variance) of a case."""
    n, M, D, fam, zl, ell, s, seed = CASES[name]
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, D))
    Y = np.sin(X[:, :1]) + 0.3 * np.cos(2 * X[:, -1:]) + 0.05 * rng.standard_normal((n, 1))
    Z = np.linspace(0, 10, M)[:, None].repeat(D, 1) if zl == "grid" else rng.uniform(0, 10, (M, D))
    gk, ok = gpx_kernel(fam), oracle_kernel(fam)
    if ell is not None:
        _set_ell(gk, ok, ell)
    return X, Y, Z, gk, ok, s


def _blocks(g):
    return {"theta": np.asarray(g["theta"]), "noise": np.asarray([g["noise"]]), "Z": np.asarray(g["Z"])}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The GPflow-route F and gradient blocks, the bars from the two routes' spread, cond(Kmm)."""
    X, Y, Z, _, ok, s = build(name)
    om = NumpySGPR(ok, X, Y, Z, noise_variance=s)
    Fa, ga = om.elbo_and_grads("gpflow")
    Fb, gb = om.elbo_and_grads("w")
    ga, gb = _blocks(ga), _blocks(gb)
    tolF = max(10.0 * abs(Fa - Fb), 1e-12 * abs(Fa))
    tolg = {k: max(10.0 * float(np.abs(ga[k] - gb[k]).max()), 1e-10 * (1.0 + float(np.abs(ga[k]).max())))
            for k in ga}
    return dict(F=Fa, g=ga, tolF=tolF, tolg=tolg, cond=float(np.linalg.cond(om.kmm())),
                spreadF=abs(Fa - Fb), spreadg={k: float(np.abs(ga[k] - gb[k]).max()) for k in ga})


def model(name):
    X, Y, Z, gk, _, s = build(name)
    return gpx.models.SGPR((X, Y), kernel=gk, inducing_variable=Z, noise_variance=s)


def _check_device(name):
    ref = reference(name)
    m = model(name)
    F, gth, gZ = m._elbo_and_grads()
    np_ = len(ref["g"]["theta"])
    got = {"theta": gth[:np_], "noise": gth[np_:np_ + 1], "Z": gZ}
    print(f"{name}: cond={ref['cond']:.3g} F={ref['F']:.17g} dF={abs(F - ref['F']):.3g} tolF={ref['tolF']:.3g}")
    for k in got:
        err = float(np.abs(got[k] - ref["g"][k]).max())
        print(f"  {k}: err={err:.3g} tol={ref['tolg'][k]:.3g} max|g|={np.abs(ref['g'][k]).max():.3g}")
    assert np.all(gth[np_ + 1:] == 0.0)
    assert abs(F - ref["F"]) <= ref["tolF"], (name, F, ref["F"], ref["tolF"])
    for k in got:
        err = float(np.abs(got[k] - ref["g"][k]).max())
        assert err <= ref["tolg"][k], (name, k, err, ref["tolg"][k])


@pytest.mark.parametrize("name", WELL)
def test_bound_and_gradients_vs_restatement(name):
    ref = reference(name)
    assert ref["cond"] <= 1e5, (name, ref["cond"])
    assert ref["tolF"] <= 1e-8 * abs(ref["F"]), (name, ref["tolF"], ref["F"])
    for k, t in ref["tolg"].items():
        assert t <= 1e-6 * (1.0 + float(np.abs(ref["g"][k]).max())), (name, k, t)
    _check_device(name)


def test_bound_and_gradients_ill_conditioned_grid():
    """The reference's inducing layout (np.linspace grid) with a long lengthscale: Kmm is nearly
    singular (cond ~ 1e8 with the jitter) and the bar is the case's own measured spread."""
    assert reference("ill")["cond"] > 1e5
    _check_device("ill")


@pytest.mark.parametrize("name", ["ref", "mp128"])  # Mp = 64 and Mp = 128
def test_predict_f_and_predict_y(name):
    """Bars as for the bound: 10x the two routes' spread, floor 1e-10 · (1 + max|ref|)."""
    X, Y, Z, _, ok, s = build(name)
    om = NumpySGPR(ok, X, Y, Z, noise_variance=s)
    D = X.shape[1]
    xs = np.random.default_rng(8).uniform(-1, 11, (333, D))
    (mo, vo), (mw, vw) = om.predict_f(xs, "gpflow"), om.predict_f(xs, "w")
    m = model(name)
    mu, var = m.predict_f(xs)
    assert tuple(mu.shape) == (333, 1) and tuple(var.shape) == (333, 1) and not mu.is_cuda
    for got, a, b in ((mu.numpy(), mo, mw), (var.numpy(), vo, vw)):
        tol = max(10.0 * float(np.abs(a - b).max()), 1e-10 * (1.0 + float(np.abs(a).max())))
        err = float(np.abs(got - a).max())
        print(f"{name}: predict err={err:.3g} tol={tol:.3g}")
        assert err <= tol, (name, err, tol)
    my, vy = m.predict_y(xs)
    np.testing.assert_array_equal(my.numpy(), mu.numpy())
    np.testing.assert_allclose(vy.numpy() - var.numpy(), s, rtol=1e-9)
    mu0, var0 = m.predict_f(np.zeros((0, D)))  # empty Xnew: empty outputs
    assert tuple(mu0.shape) == (0, 1) and tuple(var0.shape) == (0, 1)


def test_scipy_fit_of_reference_cell_matches_restatement_fit():
    """The reference's cell: Scipy().minimize(model.training_loss, model.trainable_variables) with
    the bound method, every variable trainable; the fitted loss against scipy's L-BFGS-B driven by
    the restatement from the same start."""
    X, Y, Z, _, ok, s = build("ref")
    m = model("ref")
    res = gpx.optimizers.Scipy().minimize(m.training_loss, m.trainable_variables)
    om = NumpySGPR(ok, X, Y, Z, noise_variance=s)

    def f(u):
        om.set_u(u)
        return om.loss_and_grad_u()

    ref = scipy.optimize.minimize(f, om.get_u(), jac=True, method="L-BFGS-B")
    print(f"fit: device {res.fun:.12g} in {res.nit} its, restatement {ref.fun:.12g} in {ref.nit} its")
    assert res.fun == pytest.approx(ref.fun, rel=1e-6)
    assert float(m.training_loss()) == pytest.approx(res.fun, rel=1e-12)


def test_kmm_not_positive_definite_raises():
    """Duplicate inducing points under a kernel variance of 2^40: the 1e-6 jitter is below half an
    ulp of the diagonal, so the second pivot is exactly 0."""
    X, Y, _, _, _, _ = build("ref")
    k = gpx.kernels.SquaredExponential(variance=2.0 ** 40)
    m = gpx.models.SGPR((X, Y), kernel=k, inducing_variable=np.array([[1.0], [1.0], [3.0]]))
    with pytest.raises(gpx.NotPositiveDefiniteError) as e:
        m.training_loss()
    assert e.value.info == 2
    with pytest.raises(gpx.NotPositiveDefiniteError):
        m.predict_f(X)
