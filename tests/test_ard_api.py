"""ARD (vector) lengthscales: the Python surface, the compiled spec and the θ layout, on the CPU;
and the CPU restatement the GPU tests compare against (tests/ard_numpy.py): its values against the
oracle on pre-scaled inputs, its autograd gradient against central differences on u (SURVEY §8c:
agreement <= 1e-5 relative) for every case tests/test_ard_gpu.py uses."""
import numpy as np
import pytest

import portfoliooptgp_amd as gpx
from portfoliooptgp_amd import _native as N
from portfoliooptgp_amd.kernels import compile_spec
from portfoliooptgp_amd.optimizers import _pack, _unpack
from portfoliooptgp_amd.parameter import ArrayParameter, VectorParameter, sigmoid, softplus, softplus_inverse
from tests import ard_numpy as A

K = gpx.kernels
ARD = N.GPX_TERM_ARD
STATIONARY = [K.SquaredExponential, K.Matern12, K.Matern32, K.Matern52, K.Exponential, K.RationalQuadratic]


def _xy(n=12, D=3, seed=0):
    rng = np.random.default_rng(seed)
    return rng.standard_normal((n, D)), rng.standard_normal((n, 1))


# ---------------------------------------------------------------------------- construction
@pytest.mark.parametrize("cls", STATIONARY)
def test_construction_ard_flag_and_shapes(cls):
    iso = cls(lengthscales=2.0)
    assert iso.ard is False and not isinstance(iso.lengthscales, VectorParameter)
    assert iso.lengthscales.unconstrained_variable.shape == ()
    k = cls(lengthscales=[0.5, 1.0, 2.5])
    assert k.ard is True
    ls = k.lengthscales
    assert isinstance(ls, VectorParameter) and not isinstance(ls, ArrayParameter)
    assert ls.shape == (3,) and ls.value.shape == (3,)
    np.testing.assert_allclose(ls.numpy(), [0.5, 1.0, 2.5], rtol=1e-15)
    assert ls.unconstrained_variable.shape == (3,) and ls.trainable
    k2 = cls(lengthscales=np.array([1.0, 2.0]), active_dims=[1, 2])
    assert k2.ard and k2.lengthscales.shape == (2,)
    assert "lengthscales=[0.5, 1, 2.5]" in repr(k)


def test_assign_and_softplus_round_trip_per_entry():
    k = K.SquaredExponential(lengthscales=[0.5, 1.0, 2.5])
    ls = k.lengthscales
    ls.assign(np.array([3.0, 1e-3, 40.0]))
    u = ls.unconstrained
    for d, t in enumerate([3.0, 1e-3, 40.0]):
        assert u[d] == softplus_inverse(t)
        assert ls.value[d] == softplus(u[d])
        assert ls.value[d] == pytest.approx(t, rel=1e-14)
        assert ls.dtheta_du()[d] == sigmoid(u[d])
    v = ls.unconstrained_variable
    v.assign(u + 0.25)
    np.testing.assert_array_equal(v.numpy(), u + 0.25)
    np.testing.assert_array_equal(ls.value, [softplus(x) for x in (u + 0.25)])
    with pytest.raises(ValueError):
        ls.assign([1.0, 2.0])            # wrong length
    with pytest.raises(ValueError):
        ls.assign([1.0, -2.0, 1.0])      # not positive
    with pytest.raises(ValueError):
        K.Matern32(lengthscales=[1.0, 0.0])
    with pytest.raises(ValueError):
        K.Matern32(lengthscales=[[1.0, 2.0]])


def test_parameter_order_and_paths():
    k = K.Matern52(lengthscales=[1.0, 2.0])
    assert k.parameters == (k.lengthscales, k.variance)
    assert [n for n, _ in k._param_paths("")] == ["lengthscales", "variance"]
    rq = K.RationalQuadratic(lengthscales=[1.0, 2.0, 3.0], alpha=0.7, variance=1.9)
    assert rq.parameters == (rq.alpha, rq.lengthscales, rq.variance)
    assert [n for n, _ in rq._param_paths("")] == ["alpha", "lengthscales", "variance"]
    assert rq.theta_values() == pytest.approx([0.7, 1.0, 2.0, 3.0, 1.9], rel=1e-14)
    prod = K.Exponential(lengthscales=[1.0] * 4, active_dims=[0, 1, 2, 3]) * K.Exponential(active_dims=[4])
    assert [n for n, _ in prod._param_paths("")] == [
        "kernels[0].lengthscales", "kernels[0].variance", "kernels[1].lengthscales", "kernels[1].variance"]
    X, Y = _xy(D=5)
    m = gpx.models.GPR((X, Y), kernel=prod)
    assert [n for n, _ in m._param_paths()] == [
        "GPR.kernel.kernels[0].lengthscales", "GPR.kernel.kernels[0].variance",
        "GPR.kernel.kernels[1].lengthscales", "GPR.kernel.kernels[1].variance", "GPR.likelihood.variance"]
    assert len(m.trainable_variables) == 5 and m.trainable_variables[0].shape == (4,)


# ---------------------------------------------------------------------------- compiled spec
def test_compile_spec_se_ard():
    s = compile_spec(K.SquaredExponential(lengthscales=[1.0, 2.0, 3.0]), 3)
    t = s.terms[0]
    assert s.n_terms == 1 and s.n_params == 4
    assert (t.kind, t.dim_start, t.dim_count, t.param_offset) == (N.GPX_SE | ARD, 0, 3, 0)


def test_compile_spec_rq_ard():
    s = compile_spec(K.RationalQuadratic(lengthscales=[1.0, 2.0], active_dims=[1, 2]), 4)
    t = s.terms[0]
    assert s.n_params == 4  # alpha, l0, l1, variance
    assert (t.kind, t.dim_start, t.dim_count, t.param_offset) == (N.GPX_RQ | ARD, 1, 2, 0)


def test_compile_spec_composite():
    k = K.Exponential(lengthscales=[1.0] * 4, active_dims=[0, 1, 2, 3]) * K.Exponential(active_dims=[4])
    s = compile_spec(k, 5)
    assert s.n_terms == 2 and s.combine == N.GPX_PRODUCT and s.n_params == 7
    t0, t1 = s.terms[0], s.terms[1]
    assert (t0.kind, t0.dim_start, t0.dim_count, t0.param_offset) == (N.GPX_EXPONENTIAL | ARD, 0, 4, 0)
    assert (t1.kind, t1.dim_start, t1.dim_count, t1.param_offset) == (N.GPX_EXPONENTIAL, 4, 1, 5)


def test_ard_over_one_dim_is_the_plain_term():
    for k in (K.Matern32(lengthscales=[2.0]), K.Matern32(lengthscales=[2.0], active_dims=[1])):
        assert k.ard and k.lengthscales.shape == (1,)
        D = 1 if k.active_dims is None else 3
        s, s0 = compile_spec(k, D), compile_spec(K.Matern32(lengthscales=2.0, active_dims=k.active_dims), D)
        assert bytes(s) == bytes(s0) and s.terms[0].kind == N.GPX_MATERN32
    X, Y = _xy(D=1)
    m = gpx.models.GPR((X, Y), kernel=K.Matern32(lengthscales=[2.0]))
    m0 = gpx.models.GPR((X, Y), kernel=K.Matern32(lengthscales=2.0))
    np.testing.assert_array_equal(m.theta_row(), m0.theta_row())
    assert m.trainable_variables[0].shape == (1,)


def test_theta_row_and_layout():
    X, Y = _xy(D=3)
    k = K.RationalQuadratic(lengthscales=[0.5, 1.5, 2.5], alpha=0.7, variance=1.9)
    m = gpx.models.GPR((X, Y), kernel=k, noise_variance=0.3)
    row = m.theta_row()
    np.testing.assert_allclose(row[:6], [0.7, 0.5, 1.5, 2.5, 1.9, 0.3], rtol=1e-14)
    assert m.n_kernel_params == 5
    cols, lower, tcode = m.theta_layout(m.trainable_variables, transforms=True)
    np.testing.assert_array_equal(cols, [0, 1, 2, 3, 4, 5])           # consecutive columns
    assert not tcode.any() and N.TRANSFORM_SOFTPLUS == 0              # every entry softplus
    np.testing.assert_array_equal(lower, [0, 0, 0, 0, 0, 1e-6])       # lower bound 0 for each ℓ_d
    # only the vector trainable: its three columns
    cols2, lower2 = m.theta_layout((k.lengthscales.unconstrained_variable,))
    np.testing.assert_array_equal(cols2, [1, 2, 3])
    np.testing.assert_array_equal(lower2, [0, 0, 0])
    # the optimiser's flattening: one array variable of shape (3,)
    x = _pack(m.trainable_variables)
    assert x.shape == (6,)
    np.testing.assert_array_equal(x[1:4], k.lengthscales.unconstrained)
    _unpack(m.trainable_variables, x + 0.5)
    np.testing.assert_array_equal(k.lengthscales.unconstrained, x[1:4] + 0.5)
    assert m.theta_row()[2] == softplus(x[2] + 0.5)


def test_chain_rule_uses_each_entrys_sigmoid():
    X, Y = _xy(D=2)
    k = K.SquaredExponential(lengthscales=[0.5, 4.0])
    m = gpx.models.GPR((X, Y), kernel=k)
    gth = np.arange(1.0, 17.0)
    _, g = m.loss_and_grad_unconstrained(lml=0.0, grad_theta=gth)
    u = k.lengthscales.unconstrained
    want = [-1.0 * sigmoid(u[0]), -2.0 * sigmoid(u[1]), -3.0 * k.variance.dtheta_du(),
            -4.0 * m.likelihood.variance.dtheta_du()]
    np.testing.assert_array_equal(g, want)


def test_length_mismatch_is_a_value_error():
    with pytest.raises(ValueError):
        K.SquaredExponential(lengthscales=[1.0, 2.0], active_dims=[0, 1, 2])
    with pytest.raises(ValueError):
        compile_spec(K.SquaredExponential(lengthscales=[1.0, 2.0]), 3)
    X, Y = _xy(D=3)
    with pytest.raises(ValueError):
        gpx.models.GPR((X, Y), kernel=K.Matern12(lengthscales=[1.0, 2.0]))
    with pytest.raises(ValueError):
        compile_spec(K.Exponential(lengthscales=[1.0, 2.0], active_dims=slice(1, None)), 4)


def test_row_overflow_is_refused():
    compile_spec(K.SquaredExponential(lengthscales=[1.0] * 13), 13)  # 13 + σ² + noise: accepted
    with pytest.raises(NotImplementedError) as e:
        compile_spec(K.SquaredExponential(lengthscales=[1.0] * 14), 14)
    assert str(N.GPX_THETA_STRIDE) in str(e.value)  # says how many values the row holds
    # the mean coefficients count too, as GPR.__init__ counts them
    X, Y = _xy(n=20, D=13)
    with pytest.raises(ValueError) as e2:
        gpx.models.GPR((X, Y), kernel=K.SquaredExponential(lengthscales=[1.0] * 13),
                       mean_function=gpx.mean_functions.Linear(A=np.zeros((13, 1))))
    assert str(N.GPX_THETA_STRIDE) in str(e2.value)
    gpx.models.GPR((X, Y), kernel=K.SquaredExponential(lengthscales=[1.0] * 13),
                   mean_function=gpx.mean_functions.Constant())


def test_not_provided_raises_at_construction():
    with pytest.raises(NotImplementedError):
        K.Periodic(K.SquaredExponential(lengthscales=[1.0, 2.0]))
    with pytest.raises(NotImplementedError):
        K.Linear(variance=[1.0, 2.0])
    X, Y = _xy(n=30, D=2)
    ard = lambda: K.SquaredExponential(lengthscales=[1.0, 2.0])  # noqa: E731
    Z = X[:5].copy()
    with pytest.raises(NotImplementedError):
        gpx.models.SVGP(kernel=ard(), likelihood=gpx.likelihoods.Gaussian(), inducing_variable=Z, num_data=30)
    with pytest.raises(NotImplementedError):
        gpx.models.SGPR((X, Y), kernel=ard(), inducing_variable=Z)
    with pytest.raises(NotImplementedError):
        gpx.models.VGP((X, Y), kernel=ard(), likelihood=gpx.likelihoods.Gaussian())


def test_print_summary_prints_the_vector(capsys):
    X, Y = _xy(D=3)
    m = gpx.models.GPR((X, Y), kernel=K.Matern52(lengthscales=[0.5, 1.5, 2.5]))
    gpx.utilities.print_summary(m)
    out = capsys.readouterr().out
    line = [ln for ln in out.splitlines() if "GPR.kernel.lengthscales" in ln][0]
    assert "(3,)" in line and "[0.5 1.5 2.5]" in line and "Softplus" in line
    gpx.set_trainable(m.kernel.lengthscales, False)
    assert len(m.trainable_variables) == 2


def test_series_cost_is_dense_for_ard():
    from portfoliooptgp_amd import distributed as dist
    x = np.arange(1024.0)[:, None] * np.ones((1, 2))
    assert dist.series_cost(x, K.SquaredExponential(lengthscales=[1.0, 1.0])) == dist.fit_cost(1024)
    assert dist.series_cost(x[:, :1], K.SquaredExponential(lengthscales=[1.0])) == dist.series_cost(x[:, :1])


# ---------------------------------------------------------------------------- the CPU restatement
@pytest.mark.parametrize("c", A.PARITY_CASES, ids=A.case_id)
def test_restatement_matches_oracle_and_central_differences(c):
    """The reference of tests/test_ard_gpu.py, case by case: the torch restatement's loss equals the
    oracle's on pre-scaled inputs, and its autograd gradient agrees with central differences on u
    within 1e-5 relative (noise trainable; the frozen-noise gradient is its first entries)."""
    t = A.TorchARD(c)
    loss, g = t.loss_and_grad()
    ref = A.oracle_values(c, [])
    assert abs(loss - ref["loss"]) <= 1e-9 * max(1.0, abs(ref["loss"])) * max(1.0, 1e-5 * ref["cond"])
    cd = t.central_differences()
    assert np.abs(g - cd).max() <= 1e-5 * np.abs(g).max(), (g, cd)
    # the package's flat variable order is the restatement's
    m = A.gpx_model(c)
    np.testing.assert_allclose(_pack(m.trainable_variables), t.u0, rtol=1e-13, atol=1e-13)
    g_fixed = A.TorchARD(c, trainable_noise=False).loss_and_grad()[1]
    np.testing.assert_allclose(g_fixed, g[:-1], rtol=1e-12, atol=1e-12 * np.abs(g).max())


def test_relevance_fit_on_the_restatement():
    """The end-to-end case: the restatement's own L-BFGS-B fit gives the irrelevant column the
    largest lengthscale with a clear margin (the GPU test asserts the same of the device fit)."""
    import scipy.optimize
    X, Y = A.relevance_data()
    c = A.case([("se", 0, 3, [1.0, 1.0, 1.0], 1.0, None)], len(X), 3, 1.0)
    t = A.TorchARD(c, data=(X, Y))
    r = scipy.optimize.minimize(lambda u: t.loss_and_grad(u), t.u0, jac=True, method="L-BFGS-B",
                                options=dict(maxiter=200))
    ell = np.logaddexp(0.0, r.x[:3])
    assert ell[2] > 3.0 * max(ell[0], ell[1]), ell
