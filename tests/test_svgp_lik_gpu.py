"""SVGP's per-point route on the GPU (libgpx.so gpx_svgp_create_lik: Gaussian or StudentT
likelihood) against the CPU restatement (tests/svgp_lik_numpy.py) and against the closed-form
Gaussian path of gpx_svgp_create on the same device.

Parity bars are the SGPR / VGP rule (tests/svgp_lik_cases.py): per case 10x the spread between the
restatement's two routes, floors 1e-12·|F| and 1e-10·(1 + max|g|) per block, and no case may need
more than 1e-7·|F| or 1e-5·(1 + max|g|) — asserted on the restatement before the device is looked
at. Bars of the cases as the CPU gives them (relative to |F| / to 1 + max|g|), with cond(Kmm):

    case      cond     F        theta    lik      Z        q_mu     q_sqrt
    tiny      1.0      1e-12    1e-10    1e-10    1e-10    1e-10    1e-10
    m1        1.0      1e-12    1e-10    1e-10    1e-10    1e-10    1e-10
    multi     2.7e5    4.3e-12  1e-10    1e-10    3.9e-9   1e-10    1e-10
    leaf      2.3e7    1.9e-10  2.3e-9   1.2e-10  1.7e-7   5.6e-10  3.3e-8
    mp128     4.7e1    1e-12    1e-10    1e-10    1e-10    1e-10    1e-10
    node      4.5e1    1e-12    1e-10    1e-10    1e-10    1e-10    1e-10
    chunks    6.2e6    6.3e-11  5.3e-10  1e-10    1.1e-8   3.3e-10  1.5e-9
    illcond   7.0e7    6.7e-9   2.6e-8   6.0e-9   6.8e-9   2.7e-8   1.4e-8

g_v is positive on 2.5 % to 17.5 % of the rows of the outlier cases (m1, multi, mp128, chunks).

Device errors measured on one MI355X, the worst block of each case as a fraction of its bar:
tiny 4e-6, m1 1e-5, mp128 5e-4 and node 4e-4 (the floors are the bar there); multi 0.50 (Z), leaf
0.58 (q_mu), chunks 0.63 (theta), illcond 0.23 (q_sqrt), where the bar is the references' spread and
the device is a third rounding of the same ill-conditioned products. The two device routes with the
Gaussian likelihood: |ΔF| / |F| 7e-12, 2e-16, 2e-16; blocks at most 3e-10·(1 + max|g|). The fitted
loss equals the restatement's fit to the last digit printed (140.6587887739658, 30 iterations each).
"""
import numpy as np
import pytest
import scipy.optimize

pytestmark = pytest.mark.gpu

import portfoliooptgp_amd as gpx  # noqa: E402
from portfoliooptgp_amd import _native as N  # noqa: E402
from portfoliooptgp_amd.engine import SVGPEngine  # noqa: E402
from portfoliooptgp_amd.kernels import compile_spec  # noqa: E402
from tests import svgp_lik_cases as C  # noqa: E402
from tests.svgp_lik_numpy import BLOCKS, NumpySVGPLik  # noqa: E402
from tests.test_gpu_parity import gpx_kernel  # noqa: E402


def device_kernel(name):
    gk = gpx_kernel(C.CASES[name][3])
    ell = C.build(name)[7]
    if ell is not None:
        gk.lengthscales.assign(ell)
    return gk


def model(name, likelihood=None):
    X, Y, Z, q, R, _, num_data, _ = C.build(name)
    lik = gpx.likelihoods.StudentT(scale=C.SCALE, df=C.CASES[name][6]) if likelihood is None else likelihood
    m = gpx.models.SVGP(kernel=device_kernel(name), likelihood=lik, inducing_variable=Z, num_data=num_data,
                        q_mu=q, q_sqrt=R[None], per_point=True)
    return m, X, Y


def _blocks(out, np_):
    F, gth, gZ, gq, gR = out
    assert np.all(gth[np_ + 1:] == 0.0)
    assert np.all(np.triu(gR, 1) == 0.0)
    return F, {"theta": gth[:np_], "lik": gth[np_:np_ + 1], "Z": gZ, "q_mu": gq, "q_sqrt": gR}


def _compare(name, F, got, ref):
    print(f"{name}: cond={ref['cond']:.3g} F={ref['F']:.17g} dF={abs(F - ref['F']):.3g} tolF={ref['tolF']:.3g} "
          f"spreadF={ref['spreadF']:.3g}")
    errs = {k: float(np.abs(np.asarray(got[k]).reshape(ref["g"][k].shape) - ref["g"][k]).max()) for k in BLOCKS}
    for k in BLOCKS:
        print(f"  {k}: err={errs[k]:.3g} tol={ref['tolg'][k]:.3g} spread={ref['spreadg'][k]:.3g} "
              f"max|g|={np.abs(ref['g'][k]).max():.3g}")
    assert abs(F - ref["F"]) <= ref["tolF"], (name, F, ref["F"], ref["tolF"])
    for k in BLOCKS:
        assert errs[k] <= ref["tolg"][k], (name, k, errs[k], ref["tolg"][k])


@pytest.mark.parametrize("name", list(C.CASES))
def test_elbo_and_gradients_vs_restatement(name):
    ref = C.reference(name)
    C.assert_inside_caps(name, ref)
    if C.CASES[name][5]:   # the outlier rows: g_v takes both signs, G_w is no SYRK
        assert (ref["g_v"] > 0).any() and (ref["g_v"] < 0).any()
    m, X, Y = model(name)
    F, got = _blocks(m._elbo_and_grads((X, Y)), len(m.kernel.parameters))
    _compare(name, F, got, ref)


@pytest.mark.parametrize("name", ["multi", "mp128", "chunks"])
def test_gaussian_by_the_per_point_route_equals_the_closed_form_path(name):
    """gpx_svgp_create_lik(GPX_LIK_GAUSSIAN) against gpx_svgp_create on the same device: the same
    ELBO by two launch sequences. The bound (1e-10 on F, 1e-8 per block) is summation order, and that
    holds only where Kmm is well conditioned: the closed form takes Σv = Σk_nn + tr((S − I)·W G Wᵀ),
    the per-point route Σ_n Σ_m Kmn∘(Wᵀ(S − I)W·Kmn), two roundings of W-products that each carry
    eps·cond(Kmm). So the three shapes must have 2⁻⁵²·cond(Kmm) <= 1e-10, asserted on the host
    first. "multi" (cond 2.7e5) and "mp128" (47) have it as they are. The two-chunk shape, the
    one that exercises G_w's chunk sum here, has cond 6.2e6 with its uniformly drawn Z (measured
    difference of the two routes there: 1.8e-10·|F|): this test gives it a regular grid of inducing
    points and lengthscale 0.5, about the grid's spacing."""
    X, Y, Z, q, R, ok, num_data, _ = C.build(name)
    gk = device_kernel(name)
    if name == "chunks":
        Z = np.linspace(0, 10, len(Z))[:, None]
        gk.lengthscales.assign(0.5)
        ok.lengthscales.value = 0.5
    M, D = Z.shape
    cond = float(np.linalg.cond(ok.K(Z) + 1e-6 * np.eye(M)))
    assert 2.0 ** -52 * cond <= 1e-10, (name, cond)
    spec = compile_spec(gk, D)
    np_ = len(gk.parameters)
    theta = np.ones(N.GPX_THETA_STRIDE)
    theta[:np_] = [p.value for p in gk.parameters]
    theta[np_] = 0.05
    closed = SVGPEngine(X, Y, spec, M, num_data=num_data)
    general = SVGPEngine(X, Y, spec, M, num_data=num_data, likelihood=N.GPX_LIK_GAUSSIAN, per_point=True)
    assert not closed.per_point and general.per_point
    Fa, ga = _blocks(closed.elbo_grad(theta, Z, q, R), np_)
    Fb, gb = _blocks(general.elbo_grad(theta, Z, q, R), np_)
    print(f"{name}: cond={cond:.3g} F {Fa:.17g} / {Fb:.17g} rel {abs(Fa - Fb) / abs(Fa):.3g}")
    assert abs(Fa - Fb) <= 1e-10 * abs(Fa)
    for k in BLOCKS:
        err = float(np.abs(np.asarray(ga[k]) - np.asarray(gb[k])).max())
        print(f"  {k}: err={err:.3g} max|g|={np.abs(ga[k]).max():.3g}")
        assert err <= 1e-8 * (1.0 + float(np.abs(ga[k]).max())), (name, k, err)


def test_predict_f_and_predict_y():
    name = "mp128"
    m, X, Y = model(name)
    om, _, _ = C.restatement(name)
    df = C.CASES[name][6]
    xs = np.random.default_rng(8).uniform(-1, 11, (333, 2))
    mu, var = m.predict_f(xs)
    mo, vo = om.predict_f(xs)
    assert tuple(mu.shape) == (333, 1) and tuple(var.shape) == (333, 1) and not mu.is_cuda
    assert np.abs(mu.numpy() - mo).max() <= 1e-7 * np.abs(mo).max() + 1e-10
    assert np.abs(var.numpy() - vo).max() <= 1e-7 * np.abs(vo).max() + 1e-10
    my, vy = m.predict_y(xs)
    myo, vyo = om.predict_y(xs)
    assert np.abs(my.numpy() - myo).max() <= 1e-7 * np.abs(myo).max() + 1e-10
    assert np.abs(vy.numpy() - vyo).max() <= 1e-7 * np.abs(vyo).max() + 1e-10
    np.testing.assert_allclose(vy.numpy() - var.numpy(), C.SCALE ** 2 * df / (df - 2.0), rtol=1e-9)
    np.testing.assert_array_equal(my.numpy(), mu.numpy())
    mu0, var0 = m.predict_y(np.zeros((0, 2)))  # empty Xnew: empty outputs
    assert tuple(mu0.shape) == (0, 1) and tuple(var0.shape) == (0, 1)
    # an evaluation after a predict_y still reads the scale, not the variance predict_y put in its slot
    F, got = _blocks(m._elbo_and_grads((X, Y)), len(m.kernel.parameters))
    _compare(name + "/after predict_y", F, got, C.reference(name))


def test_sharded_partials_equal_single_shard():
    """Two per-point shards' partial buffers summed (what the all-reduce does) then finished equal
    the unsharded evaluation — the multi-GPU decomposition, on one device."""
    rng = np.random.default_rng(9)
    n, M = 3001, 77
    X = rng.uniform(0, 10, (n, 1))
    Y = np.sin(X) + 0.3 * np.cos(2 * X) + 0.05 * rng.standard_normal((n, 1))
    out = rng.choice(n, n // 20, replace=False)
    Y[out, 0] += rng.choice([-1.0, 1.0], len(out)) * 2.0
    Z = rng.uniform(0, 10, (M, 1))
    R = np.tril(rng.standard_normal((M, M)) * 0.05)
    R[np.diag_indices(M)] = rng.uniform(0.3, 1.0, M)
    q = rng.standard_normal(M) * 0.5
    gk = gpx_kernel("se")
    spec = compile_spec(gk, 1)
    theta = np.ones(N.GPX_THETA_STRIDE)
    theta[:2] = [p.value for p in gk.parameters]
    theta[2] = C.SCALE
    kw = dict(likelihood=N.GPX_LIK_STUDENT_T, df=3.0)
    full = SVGPEngine(X, Y, spec, M, num_data=n, **kw).elbo_grad(theta, Z, q, R)
    a = SVGPEngine(X[:1400], Y[:1400], spec, M, num_data=n, n_total=n, **kw)
    b = SVGPEngine(X[1400:], Y[1400:], spec, M, num_data=n, n_total=n, **kw)
    a.eval_local(theta, Z, q, R)
    b.eval_local(theta, Z, q, R)
    a.partials += b.partials
    got = a.eval_finish()
    # equal up to summation order (G_w, w, the θ / Z partials, Σ ve and Σ ∂ve/∂φ are split differently)
    assert got[0] == pytest.approx(full[0], rel=1e-9)
    for x, y in zip(got[1:], full[1:]):
        np.testing.assert_allclose(x, y, rtol=1e-8, atol=1e-8 * (1 + np.abs(y).max()))
    assert full[1][2] != 0.0    # the scale's gradient came through the partial buffer


def test_second_evaluation_equals_fresh_model():
    """No stale padding or workspace: after one evaluation and one predict_y, a second evaluation on
    the same model with another q, R, Z and θ gives the bits a fresh model gives."""
    name = "multi"
    M = C.CASES[name][1]
    rng = np.random.default_rng(11)
    q2 = rng.standard_normal(M)
    R2 = np.tril(0.3 * rng.standard_normal((M, M)), -1) + np.diag(rng.uniform(0.3, 1.5, M))

    def move(m):
        m.q_mu.assign(q2[:, None])
        m.q_sqrt.assign(R2[None])
        m.inducing_variable.Z.assign(m.inducing_variable.Z.value + 0.05)
        for p in m.kernel.parameters:
            p.assign(p.value * 1.3)
        m.likelihood.scale.assign(0.7)

    used, X, Y = model(name)
    used._elbo_and_grads((X, Y))
    used.predict_y(X[:7])
    move(used)
    fresh, _, _ = model(name)
    move(fresh)
    np_ = len(used.kernel.parameters)
    Fu, gu = _blocks(used._elbo_and_grads((X, Y)), np_)
    Ff, gf = _blocks(fresh._elbo_and_grads((X, Y)), np_)
    assert Fu == Ff
    for k in BLOCKS:
        np.testing.assert_array_equal(gu[k], gf[k])


def test_scipy_fit_reaches_the_restatements_fit():
    """The reference's cell shape (N = 113 day offsets in 0..360, M = 10 on np.linspace(0, 360, 10),
    SE kernel, StudentT(), everything trainable, the scale included): 30 L-BFGS-B iterations driven
    by the device end where 30 driven by the restatement end."""
    rng = np.random.default_rng(3)
    n = 113
    X = np.sort(np.concatenate([[0, 360], rng.choice(np.arange(1, 360), n - 2, replace=False)]))
    X = X.astype(np.float64)[:, None]
    Y = np.sin(X / 40.0) + 0.1 * rng.standard_normal((n, 1))
    Y[rng.choice(n, 5, replace=False), 0] += 1.0
    Z = np.linspace(0, 360, 10)[:, None]
    m = gpx.models.SVGP(kernel=gpx.kernels.SquaredExponential(), likelihood=gpx.likelihoods.StudentT(),
                        inducing_variable=Z, num_data=n, per_point=True)
    assert len(m.trainable_variables) == 6
    start = float(m.training_loss((X, Y)))
    res = gpx.optimizers.Scipy().minimize(m.training_loss_closure((X, Y)), m.trainable_variables,
                                          options=dict(maxiter=30))
    from oracle import gp_oracle as O
    om = NumpySVGPLik(O.OSquaredExponential(), Z, likelihood="studentt", scale=1.0, df=3.0, num_data=n)
    assert -om.elbo(X, Y) == pytest.approx(start, rel=1e-10)

    def f(u):
        om.set_u(u)
        return om.loss_and_grad_u(X, Y)

    ref = scipy.optimize.minimize(f, om.get_u(), jac=True, method="L-BFGS-B", options=dict(maxiter=30))
    print(f"start {start:.12g}; device fit {res.fun:.17g} in {res.nit} its; restatement fit {ref.fun:.17g} "
          f"in {ref.nit} its; scale {m.likelihood.scale.value:.6g} / {om.noise.value:.6g}")
    assert res.fun < start
    assert m.likelihood.scale.value != 1.0
    assert abs(res.fun - ref.fun) <= 1e-5 * abs(ref.fun), (res.fun, ref.fun)


def test_argument_errors():
    X, Y, Z, q, R, _, num_data, _ = C.build("tiny")
    gk = gpx_kernel("se")
    spec = compile_spec(gk, 1)
    theta = np.ones(N.GPX_THETA_STRIDE)
    theta[2] = C.SCALE
    for df in (0.0, -1.0, float("nan")):
        with pytest.raises(gpx.GPXError, match="df"):
            SVGPEngine(X, Y, spec, 3, num_data=5, likelihood=N.GPX_LIK_STUDENT_T, df=df)
    with pytest.raises(ValueError):
        SVGPEngine(X, Y, spec, 3, num_data=5, likelihood=7)
    eng = SVGPEngine(X, Y, spec, 3, num_data=5, likelihood=N.GPX_LIK_STUDENT_T, df=1.5)   # df in (0, 2]: no variance
    F = eng.elbo_grad(theta, Z, q, R)[0]
    assert np.isfinite(F)
    mu, _ = eng.predict(theta, Z, q, R, X, False)
    assert np.all(np.isfinite(mu.cpu().numpy()))
    with pytest.raises(gpx.GPXError, match="df > 2"):
        eng.predict(theta, Z, q, R, X, True)
    for bad_scale in (0.0, -0.3, float("inf"), float("nan")):
        bad = theta.copy()
        bad[2] = bad_scale
        with pytest.raises(gpx.GPXError, match=r"\(2\)"):       # GPX_BAD_ARG
            eng.elbo_grad(bad, Z, q, R)
    assert N.GPX_BAD_ARG == 2
    assert eng.elbo_grad(theta, Z, q, R)[0] == F                # and the engine still evaluates


def test_not_positive_definite_reports_the_pivot():
    """Duplicate inducing points under a kernel variance of 2^40: the 1e-6 jitter is below half an
    ulp of the diagonal, so the second pivot is exactly 0 — GPX_NOT_PD from the per-point route."""
    Z = np.array([[1.0], [1.0], [3.0]])
    X = np.linspace(0, 4, 9)[:, None]
    m = gpx.models.SVGP(kernel=gpx.kernels.SquaredExponential(variance=2.0 ** 40),
                        likelihood=gpx.likelihoods.StudentT(), inducing_variable=Z, num_data=9,
                        per_point=True)
    with pytest.raises(gpx.NotPositiveDefiniteError) as e:
        m.training_loss((X, np.zeros((9, 1))))
    assert e.value.info == 2
    with pytest.raises(gpx.NotPositiveDefiniteError):
        m.predict_f(X)
