"""ARD (vector-lengthscale) GPR on the GPU against the CPU reference of tests/ard_numpy.py: values
from the oracle on pre-scaled inputs, gradients from the torch-fp64 autograd restatement (validated
against central differences on the CPU, tests/test_ard_api.py).

Sizes: N = 5 and 60 (Np = 64), 67 (Np = 128: both on the launch chain, the ARD route of the small
sizes), 200 (Np = 256: the recursion and off-diagonal 64-tiles in the contraction), 600 (Np = 640:
the 128-tile instances). Bars of tests/test_gpu_parity.py:
  logML     (1e-9 + 1e-14 κ)·max(1, |ref|)          gradient  1e-6·max|g_ref|
  mean      1e-6·max|ref| + 1e-14 κ·max(1, max|y|)  variance  1e-5·|ref| + 1e-10·σ²_max
"""
import functools

import numpy as np
import pytest
import scipy.optimize

pytestmark = pytest.mark.gpu

import portfoliooptgp_amd as gpx  # noqa: E402
from portfoliooptgp_amd import _native as N  # noqa: E402
from portfoliooptgp_amd.engine import Engine  # noqa: E402
from portfoliooptgp_amd.kernels import compile_spec  # noqa: E402
from tests import ard_numpy as A  # noqa: E402
from tests.test_gpu_parity import check_grad, check_loss, check_mean, check_var  # noqa: E402

K = gpx.kernels


@functools.lru_cache(maxsize=None)
def _reference(i):
    """(oracle values at N* in {1, N + 1}, restatement gradient with trainable / frozen noise, the
    prediction inputs) of PARITY_CASES[i]: computed once, shared, never modified."""
    c = A.PARITY_CASES[i]
    rng = np.random.default_rng(1000 + i)
    xnews = (rng.standard_normal((1, c["D"])), rng.standard_normal((c["n"] + 1, c["D"])))
    ref = A.oracle_values(c, xnews)
    g = A.TorchARD(c).loss_and_grad()[1]
    g_fixed = A.TorchARD(c, trainable_noise=False).loss_and_grad()[1]
    return ref, g, g_fixed, xnews


@pytest.mark.parametrize("i", range(len(A.PARITY_CASES)), ids=[A.case_id(c) for c in A.PARITY_CASES])
def test_parity_at_fixed_theta(i):
    c = A.PARITY_CASES[i]
    ref, g_ref, g_fixed_ref, xnews = _reference(i)
    cond = ref["cond"]
    m = A.gpx_model(c)
    assert any(m._spec.terms[t].kind & N.GPX_TERM_ARD for t in range(m._spec.n_terms))
    loss, g = m.loss_and_grad_unconstrained()
    print(A.case_id(c), "cond", cond, "loss", loss, ref["loss"], "grad err/scale",
          np.abs(g - g_ref).max() / np.abs(g_ref).max())
    check_loss(loss, ref["loss"], cond)
    check_grad(g, g_ref)
    gpx.set_trainable(m.likelihood.variance, False)
    _, g2 = m.loss_and_grad_unconstrained()
    check_grad(g2, g_fixed_ref)
    yscale = float(np.abs(m.data[1].numpy()).max())
    for xn, (fm, fv, fc) in zip(xnews, ref["pred"]):
        s2 = max(float(np.max(fv)), 1.0)
        mu, var = m.predict_f(xn)
        check_mean(mu.numpy(), fm, cond, yscale)
        check_var(var.numpy(), fv, s2)
        _, vy = m.predict_y(xn)
        check_var(vy.numpy(), fv + c["noise"], s2)
        mu2, cov = m.predict_f(xn, full_cov=True)
        check_mean(mu2.numpy(), fm, cond, yscale)
        assert cov.shape == (1, len(xn), len(xn))
        check_var(cov.numpy()[0], fc, s2)  # (elementwise: |Δ| <= 1e-5 |ref| + 1e-10 σ²_max)


# ---------------------------------------------------------------------------- degenerate ARD
@pytest.mark.parametrize("fam,n,D", [("se", 60, 3), ("m32", 67, 2), ("exp", 200, 5), ("rq", 600, 3), ("m52", 200, 2)])
def test_equal_lengthscales_match_the_isotropic_model(fam, n, D):
    ell = 1.7
    c = A.single(fam, n, D, 1e-2, seed=50 + n, ell=[ell] * D)
    ci = A.single(fam, n, D, 1e-2, seed=50 + n, ell=ell)
    m, mi = A.gpx_model(c), A.gpx_model(ci)
    assert m._spec.terms[0].kind == mi._spec.terms[0].kind | N.GPX_TERM_ARD
    cond = A.oracle_values(c, [])["cond"]
    loss, g = m.loss_and_grad_unconstrained()
    loss_i, g_i = mi.loss_and_grad_unconstrained()
    check_loss(loss, loss_i, cond)
    # θ order: [alpha,] ℓ_0 … ℓ_{D−1}, σ², noise against [alpha,] ℓ, σ², noise; equal ℓ_d share one
    # u, so Σ_d ∂/∂u_d is the isotropic ∂/∂u
    o = 1 if fam == "rq" else 0
    summed = np.concatenate([g[:o], [g[o:o + D].sum()], g[o + D:]])
    check_grad(summed, g_i)
    xn = np.random.default_rng(3).standard_normal((n + 1, D))
    (mu, var), (mu_i, var_i) = m.predict_f(xn), mi.predict_f(xn)
    check_mean(mu.numpy(), mu_i.numpy(), cond, float(np.abs(m.data[1].numpy()).max()))
    check_var(var.numpy(), var_i.numpy(), max(float(var_i.max()), 1.0))


@pytest.mark.parametrize("n", [60, 600])
def test_one_active_dim_is_bit_identical_to_the_scalar_model(n):
    """A length-1 lengthscale vector compiles to the plain term: the same spec, the same route,
    the same bits."""
    X, Y = A.make_data(n, 3, seed=70)
    ms = [gpx.models.GPR((X, Y), kernel=K.Matern52(lengthscales=ls, variance=1.4, active_dims=[1]),
                         noise_variance=1e-2) for ls in ([0.8], 0.8)]
    assert bytes(ms[0]._spec) == bytes(ms[1]._spec)
    (l0, g0), (l1, g1) = (m.loss_and_grad_unconstrained() for m in ms)
    assert l0 == l1
    np.testing.assert_array_equal(g0, g1)
    xn = np.random.default_rng(4).standard_normal((7, 3))
    (mu0, v0), (mu1, v1) = (m.predict_f(xn) for m in ms)
    np.testing.assert_array_equal(mu0.numpy(), mu1.numpy())
    np.testing.assert_array_equal(v0.numpy(), v1.numpy())


# ---------------------------------------------------------------------------- mixed batches
def _mixed_models(ns, seed0):
    """{isotropic SE, SE-ARD, Matern52-ARD, Exp(ARD) x Exp} on D = 3 data of ragged N."""
    out = []
    for j, n in enumerate(ns):
        X, Y = A.make_data(n, 3, seed=seed0 + j)
        k = [lambda: K.SquaredExponential(lengthscales=1.3),
             lambda: K.SquaredExponential(lengthscales=[0.7, 1.4, 2.6]),
             lambda: K.Matern52(lengthscales=[2.0, 0.9, 1.5], variance=1.2),
             lambda: K.Exponential(lengthscales=[1.1, 2.2], active_dims=[0, 1]) * K.Exponential(active_dims=[2])][j % 4]()
        m = gpx.models.GPR((X, Y), kernel=k, noise_variance=1e-2)
        gpx.set_trainable(m.likelihood.variance, False)
        out.append(m)
    return out


def test_mixed_batch_fits_equal_solo_fits():
    ns = [200, 217, 234, 251]  # (one padded size: a slot's arithmetic depends on its own data and Np)
    seq = [gpx.optimizers.Scipy().minimize(m.training_loss, m.trainable_variables, options=dict(maxiter=30))
           for m in _mixed_models(ns, 80)]
    bat = gpx.optimizers.Scipy().minimize_batch(_mixed_models(ns, 80), options=dict(maxiter=30))
    for a, b in zip(seq, bat):
        assert a.nfev == b.nfev and a.nit == b.nit
        np.testing.assert_allclose(a.x, b.x, rtol=1e-10)
        assert a.fun == pytest.approx(b.fun, rel=1e-12)


def test_mixed_stream_fits_equal_solo_fits():
    """The continuous-batching driver (3 slots, 6 mixed fits rebinding slots between isotropic and
    ARD specs, the native stepper's flattened vector variable) against solo fits, with the
    tolerances of test_stream_fits_equal_solo_fits."""
    ns = [200, 217, 234, 251, 243, 222]
    solo = []
    for m in _mixed_models(ns, 120):
        r = gpx.optimizers.Scipy().minimize(m.training_loss, m.trainable_variables, options=dict(maxiter=25))
        solo.append((r, m.predict_f(m.data[0])))
    models = _mixed_models(ns, 120)
    res, preds = gpx.optimizers.Scipy().minimize_stream(models, width=3, predict_train=True, options=dict(maxiter=25))
    for (r0, (mu0, v0)), r1, (mu1, v1), m in zip(solo, res, preds, models):
        assert r0.nfev == r1.nfev
        np.testing.assert_allclose(r0.x, r1.x, rtol=1e-9)
        np.testing.assert_allclose(mu0.numpy()[:, 0], mu1.cpu().numpy()[:, 0], rtol=1e-9, atol=1e-12)
        np.testing.assert_allclose(v0.numpy()[:, 0], v1.cpu().numpy()[:, 0], rtol=1e-7, atol=1e-12)
        # the fitted vector landed in the model's parameter
        np.testing.assert_allclose(np.concatenate([np.atleast_1d(v.numpy()).ravel() for v in m.trainable_variables]),
                                   r1.x, rtol=0, atol=0)


@pytest.mark.parametrize("ns", [[5, 60, 33, 64], [67, 100, 128, 90], [200, 217, 234, 251, 256, 130, 140, 150]],
                         ids=["Np64", "Np128", "Np256"])
def test_mixed_engine_call_equals_slot_by_slot_calls(ns):
    """Engine.lml_grad at fixed θ over mixed slots: every slot's result is the one it gets alone
    (atol = 0), whichever other specs share the call; predictions likewise."""
    models = _mixed_models(ns, 90)
    eng = Engine([m.data[0] for m in models], [m.data[1] for m in models], [m._spec for m in models])
    theta = np.stack([m.theta_row() for m in models])
    B = len(models)
    lml, grad, info = eng.lml_grad(list(range(B)), theta)
    assert not info.any()
    for order in ([b] for b in range(B)):
        l1, g1, i1 = eng.lml_grad(order, theta)
        b = order[0]
        assert i1[b] == 0 and l1[b] == lml[b]
        np.testing.assert_array_equal(g1[b], grad[b])
    l2, g2, _ = eng.lml_grad(list(range(B))[::-1], theta)
    np.testing.assert_array_equal(l2, lml)
    np.testing.assert_array_equal(g2, grad)
    xs = [np.random.default_rng(b).standard_normal((9, 3)) for b in range(B)]
    m_all, v_all, _ = eng.predict(list(range(B)), theta, xs, False)
    for b in range(B):
        m1, v1, _ = eng.predict([b], theta, [xs[b]], False)
        np.testing.assert_array_equal(m1[0].cpu().numpy(), m_all[b].cpu().numpy())
        np.testing.assert_array_equal(v1[0].cpu().numpy(), v_all[b].cpu().numpy())
    # and each slot against its own model's solo engine of the same padded size
    for b, m in enumerate(models):
        if (m.data[0].shape[0] + 63) // 64 == (max(ns) + 63) // 64:
            ls, gs = m.loss_and_grad_unconstrained()
            lb, gb = m.loss_and_grad_unconstrained(lml=lml[b], grad_theta=grad[b])
            assert ls == lb
            np.testing.assert_array_equal(gs, gb)


# ---------------------------------------------------------------------------- end to end
def test_fit_finds_the_irrelevant_column():
    """N = 120, D = 3, SE-ARD, y a function of columns 0 and 1: Scipy().minimize against
    scipy's L-BFGS-B on the restatement from the same start (fun within rel 1e-5, the project's
    fit bar); the irrelevant column gets the largest fitted lengthscale (the restatement's own fit
    shows it with a factor > 3, tests/test_ard_api.py)."""
    X, Y = A.relevance_data()
    m = gpx.models.GPR((X, Y), kernel=K.SquaredExponential(lengthscales=[1.0, 1.0, 1.0]))
    res = gpx.optimizers.Scipy().minimize(m.training_loss, m.trainable_variables, options=dict(maxiter=200))
    c = A.case([("se", 0, 3, [1.0, 1.0, 1.0], 1.0, None)], len(X), 3, 1.0)
    t = A.TorchARD(c, data=(X, Y))
    ref = scipy.optimize.minimize(lambda u: t.loss_and_grad(u), t.u0, jac=True, method="L-BFGS-B",
                                  options=dict(maxiter=200))
    print("fit", res.fun, ref.fun, m.kernel.lengthscales.value)
    assert abs(res.fun - ref.fun) <= 1e-5 * abs(ref.fun), (res.fun, ref.fun)
    ell = m.kernel.lengthscales.value
    assert ell[2] > max(ell[0], ell[1])
    assert int(np.argmax(ell)) == 2


# ---------------------------------------------------------------------------- failure semantics
def test_invalid_lengthscale_raises_invalid_parameter_error():
    X, Y = A.make_data(60, 3, seed=5)
    m = gpx.models.GPR((X, Y), kernel=K.SquaredExponential(lengthscales=[1.0, 2.0, 3.0]))
    u = m.kernel.lengthscales.unconstrained.copy()
    for bad in (-1e4, np.nan, np.inf):  # softplus underflows to ℓ_1 = 0; non-finite
        ub = u.copy()
        ub[1] = bad
        m.kernel.lengthscales.set_unconstrained(ub)
        with pytest.raises(N.InvalidParameterError):
            m.training_loss()
    m.kernel.lengthscales.set_unconstrained(u)
    assert np.isfinite(float(m.training_loss()))


def test_not_positive_definite_raises_as_the_isotropic_path_does():
    """Duplicate inputs under a kernel variance of 2^40: the noise is below half an ulp of the
    diagonal, so the second pivot is exactly 0 — for the ARD spec as for the isotropic one."""
    X = np.array([[1.0, 2.0], [1.0, 2.0], [3.0, 0.5]])
    for ls in ([1.0, 2.0], 1.0):
        m = gpx.models.GPR((X, np.zeros((3, 1))), kernel=K.SquaredExponential(variance=2.0 ** 40, lengthscales=ls),
                           noise_variance=2e-6)
        with pytest.raises(N.NotPositiveDefiniteError) as e:
            m.training_loss()
        assert e.value.info == 2


def test_c_abi_refuses_misplaced_flags():
    """GPX_TERM_ARD on a kind that has no ARD form, or with one active dim: GPX_BAD_ARG with a
    gpx_last_error text (GPXError), before any device work."""
    X, Y = A.make_data(20, 3, seed=6)
    good = compile_spec(K.SquaredExponential(lengthscales=[1.0, 2.0, 3.0]), 3)
    Engine([X], [Y], [good])
    for kind, dims in ((N.GPX_LINEAR | N.GPX_TERM_ARD, 3), (N.GPX_PERIODIC_SE | N.GPX_TERM_ARD, 3),
                       (N.GPX_SE | N.GPX_TERM_ARD, 1), (N.GPX_SE | 0x200, 3)):
        bad = compile_spec(K.SquaredExponential(lengthscales=[1.0, 2.0, 3.0]), 3)
        bad.terms[0].kind = kind
        bad.terms[0].dim_count = dims
        with pytest.raises(gpx.GPXError):
            Engine([X], [Y], [bad])
    # band queries report an ARD slot as dense
    xs, ys = A.make_data(600, 2, seed=7)
    xs = np.sort(xs, axis=0) * 1000.0  # (far apart against ℓ = 1: an isotropic spec would be banded)
    e2 = Engine([xs, xs], [ys, ys], [compile_spec(K.SquaredExponential(lengthscales=[1.0, 1.0]), 2),
                                     compile_spec(K.SquaredExponential(), 2)])
    th = np.ones((2, N.GPX_THETA_STRIDE))
    if hasattr(e2, "band_width"):
        p = e2.band_width([0, 1], th)
        assert p[0] == -1
