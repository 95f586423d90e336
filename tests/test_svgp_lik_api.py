"""SVGP with the StudentT likelihood, the model surface on the CPU (no device calls): construction,
GPflow's variable order, count, paths and shapes, the scale in the θ row and through softplus in
the gradient mapping, print_summary, the engine arguments, and what the model still refuses. The
per-point route that serves StudentT is opt-in (``per_point=True``): without the keyword
``SVGP(kernel, StudentT(), Z)`` raises as it always did."""
import numpy as np
import pytest

import portfoliooptgp_amd as gpx
from portfoliooptgp_amd import _native as N


def _model(lik=None, M=5, **kw):
    Z = np.linspace(0, 10, M)[:, None]
    k = gpx.kernels.SquaredExponential(lengthscales=1.5, variance=0.7)
    return gpx.models.SVGP(kernel=k, likelihood=gpx.likelihoods.StudentT(scale=0.3, df=4.0) if lik is None else lik,
                           inducing_variable=Z, num_data=40, **{"per_point": True, **kw})


def test_construction_with_student_t():
    m = _model()
    assert isinstance(m.likelihood, gpx.likelihoods.StudentT)
    assert m.likelihood.df == 4.0 and m.likelihood.scale.value == pytest.approx(0.3)
    assert m.num_latent_gps == 1 and m.whiten is True and m.num_data == 40 and m.M == 5
    assert m.q_mu.shape == (5, 1) and np.all(m.q_mu.value == 0.0)
    np.testing.assert_array_equal(m.q_sqrt.value[0], np.eye(5))
    row = m.theta_row()
    assert row.shape == (N.GPX_THETA_STRIDE,) and tuple(row[:3]) == pytest.approx((1.5, 0.7, 0.3))
    m.likelihood.scale.assign(0.45)
    assert m.theta_row()[2] == pytest.approx(0.45)
    assert m.per_point and m._engine_likelihood() == dict(likelihood=N.GPX_LIK_STUDENT_T, df=4.0, per_point=True)
    g = _model(gpx.likelihoods.Gaussian(0.2), per_point=False)
    assert g._engine_likelihood() == dict(likelihood=N.GPX_LIK_GAUSSIAN, per_point=False)   # the closed-form path
    assert g.theta_row()[2] == pytest.approx(0.2)
    g = _model(gpx.likelihoods.Gaussian(0.2))                                # Gaussian by the general route
    assert g._engine_likelihood() == dict(likelihood=N.GPX_LIK_GAUSSIAN, per_point=True)


def test_variables_follow_gpflow_order_count_paths_and_shapes():
    m = _model()
    assert m.parameters == (m.inducing_variable.Z, m.kernel.lengthscales, m.kernel.variance,
                            m.likelihood.scale, m.q_mu, m.q_sqrt)
    assert [v.name for v in m.trainable_variables] == ["Z:0", "lengthscales:0", "variance:0", "scale:0",
                                                       "q_mu:0", "q_sqrt:0"]
    assert [tuple(v.shape) for v in m.trainable_variables] == [(5, 1), (), (), (), (5, 1), (1, 15)]
    assert [n for n, _ in m._param_paths()] == ["SVGP.inducing_variable.Z", "SVGP.kernel.lengthscales",
                                                "SVGP.kernel.variance", "SVGP.likelihood.scale",
                                                "SVGP.q_mu", "SVGP.q_sqrt"]
    assert [p for _, p in m._param_paths()] == list(m.parameters)
    gpx.set_trainable(m.likelihood.scale, False)
    assert [v.name for v in m.trainable_variables] == ["Z:0", "lengthscales:0", "variance:0", "q_mu:0", "q_sqrt:0"]
    g = _model(gpx.likelihoods.Gaussian(0.2))
    assert [n for n, _ in g._param_paths()][3] == "SVGP.likelihood.variance"
    assert g.trainable_variables[3]._param is g.likelihood.variance


def test_gradient_mapping_chains_the_scale_through_softplus():
    m = _model()
    M = 5
    rng = np.random.default_rng(0)
    gth = np.zeros(16)
    gth[:3] = [0.3, -1.2, 0.8]
    gZ, gq, gR = rng.standard_normal((M, 1)), rng.standard_normal(M), np.tril(rng.standard_normal((M, M)))
    loss, gu = m.grads_to_unconstrained(m.trainable_variables, 2.5, gth, gZ, gq, gR)
    assert loss == -2.5 and gu.shape == (M + 3 + M + M * (M + 1) // 2,)
    np.testing.assert_array_equal(gu[:M], -gZ.ravel())
    for i, p in enumerate((m.kernel.lengthscales, m.kernel.variance, m.likelihood.scale)):
        assert gu[M + i] == pytest.approx(-gth[i] * p.dtheta_du(), rel=1e-15)
    # softplus: dθ/du = sigmoid(u) = 1 − exp(−θ) at θ = 0.3 (lower bound 0)
    assert m.likelihood.scale.dtheta_du() == pytest.approx(1.0 - np.exp(-0.3), rel=1e-12)
    np.testing.assert_array_equal(gu[M + 3:M + 3 + M], -gq)
    np.testing.assert_array_equal(gpx.parameter.fill_triangular(-gu[M + 3 + M:]), gR)
    gpx.set_trainable(m.likelihood.scale, False)
    _, gu2 = m.grads_to_unconstrained(m.trainable_variables, 2.5, gth, gZ, gq, gR)
    np.testing.assert_array_equal(gu2, np.concatenate([gu[:M + 2], gu[M + 3:]]))
    assert m.training_loss_closure((np.zeros((3, 1)), np.zeros((3, 1))))._gpx_model is m


def test_print_summary_shows_the_scale(capsys):
    gpx.print_summary(_model())
    out = capsys.readouterr().out
    for name in ("SVGP.inducing_variable.Z", "SVGP.kernel.lengthscales", "SVGP.kernel.variance",
                 "SVGP.likelihood.scale", "SVGP.q_mu", "SVGP.q_sqrt"):
        assert name in out, name
    assert "SVGP.likelihood.variance" not in out and "0.3" in out and "df" not in out


def test_refusals():
    Z = np.linspace(0, 10, 5)[:, None]
    k = gpx.kernels.SquaredExponential()
    st = gpx.likelihoods.StudentT()
    pp = dict(per_point=True)
    with pytest.raises(NotImplementedError, match="Gaussian and StudentT"):
        gpx.models.SVGP(kernel=k, likelihood=object(), inducing_variable=Z, **pp)
    # the route is opt-in: without the keyword StudentT is refused, and the message names both
    # likelihoods and the keyword
    with pytest.raises(NotImplementedError, match="per_point=True.*Gaussian and StudentT"):
        gpx.models.SVGP(kernel=k, likelihood=st, inducing_variable=Z)
    with pytest.raises(NotImplementedError):
        gpx.models.SVGP(kernel=k, likelihood=st, inducing_variable=Z, q_diag=True, **pp)
    with pytest.raises(NotImplementedError):
        gpx.models.SVGP(kernel=k, likelihood=st, inducing_variable=Z, whiten=False, **pp)
    with pytest.raises(NotImplementedError):
        gpx.models.SVGP(kernel=k, likelihood=st, inducing_variable=Z, mean_function=gpx.mean_functions.Constant(),
                        **pp)
    with pytest.raises(NotImplementedError):
        gpx.models.SVGP(kernel=k, likelihood=st, inducing_variable=Z, num_latent_gps=2, **pp)
    with pytest.raises(NotImplementedError, match="ARD"):
        gpx.models.SVGP(kernel=gpx.kernels.SquaredExponential(lengthscales=[1.0, 2.0]), likelihood=st,
                        inducing_variable=np.zeros((5, 2)), **pp)
    m = gpx.models.SVGP(kernel=k, likelihood=st, inducing_variable=Z, **pp)
    for f in (m.predict_f, m.predict_y):
        with pytest.raises(NotImplementedError):
            f(Z, full_cov=True)
    with pytest.raises(ValueError):
        gpx.likelihoods.StudentT(df=2.0)    # predict_y's variance needs df > 2: refused at construction


def test_symbol_is_bound():
    assert "gpx_svgp_create_lik" in N.EXPORTED_SYMBOLS
    fn = N.load_library().gpx_svgp_create_lik     # loading needs no device
    assert len(fn.argtypes) == len(N.load_library().gpx_svgp_create.argtypes) + 2
