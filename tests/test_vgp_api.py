"""VGP model surface on the CPU (no device calls): GPflow variable order, paths and shapes, the
StudentT likelihood, the constrained → unconstrained gradient mapping, what the model refuses,
and print_summary."""
import numpy as np
import pytest
import torch

import portfoliooptgp_amd as gpx
from portfoliooptgp_amd import _native as N


def _data(n=9, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, 1))
    return X, np.sin(X) + 0.1 * rng.standard_normal((n, 1))


def _model(lik=None, n=9, **kw):
    X, Y = _data(n)
    k = gpx.kernels.SquaredExponential(lengthscales=1.5, variance=0.7)
    return gpx.models.VGP((X, Y), kernel=k, likelihood=gpx.likelihoods.StudentT() if lik is None else lik, **kw)


def test_student_t_defaults_and_parameters():
    lik = gpx.likelihoods.StudentT()
    assert lik.scale.value == pytest.approx(1.0) and lik.df == 3.0 and isinstance(lik.df, float)
    assert lik.parameters == (lik.scale,)          # df is not a parameter
    assert lik.scale.lower == 0.0 and lik.scale.transform_name == "Softplus"
    assert [v.name for v in lik.trainable_variables] == ["scale:0"]
    lik = gpx.likelihoods.StudentT(scale=0.25, df=5)
    assert lik.scale.value == pytest.approx(0.25) and lik.df == 5.0
    for df in (2.0, 1.0, 0.0, -3.0, float("nan")):
        with pytest.raises(ValueError):
            gpx.likelihoods.StudentT(df=df)
    with pytest.raises(ValueError):
        gpx.likelihoods.StudentT(scale=0.0)


def test_vgp_is_exported_with_gpflow_attributes():
    m = _model()
    assert gpx.models.VGP is type(m)
    assert m.num_latent_gps == 1 and m.num_data == 9
    assert isinstance(m.likelihood, gpx.likelihoods.StudentT)
    assert tuple(m.data[0].shape) == (9, 1) and tuple(m.data[1].shape) == (9, 1)
    assert m.data[0].dtype == torch.float64
    assert m.q_mu.shape == (9, 1) and np.all(m.q_mu.value == 0.0)
    assert m.q_sqrt.shape == (1, 9, 9)
    np.testing.assert_array_equal(m.q_sqrt.value[0], np.eye(9))
    for name in ("elbo", "maximum_log_likelihood_objective", "training_loss", "training_loss_closure",
                 "loss_and_grad_unconstrained", "predict_f", "predict_y"):
        assert callable(getattr(m, name))
    row = m.theta_row()
    assert row.shape == (N.GPX_THETA_STRIDE,) and tuple(row[:3]) == pytest.approx((1.5, 0.7, 1.0))


def test_vgp_variables_follow_gpflow_order_paths_and_shapes():
    m = _model()
    assert m.parameters == (m.kernel.lengthscales, m.kernel.variance, m.likelihood.scale, m.q_mu, m.q_sqrt)
    assert [v.name for v in m.trainable_variables] == ["lengthscales:0", "variance:0", "scale:0", "q_mu:0",
                                                       "q_sqrt:0"]
    assert [tuple(v.shape) for v in m.trainable_variables] == [(), (), (), (9, 1), (1, 9 * 10 // 2)]
    assert [n for n, _ in m._param_paths()] == ["VGP.kernel.lengthscales", "VGP.kernel.variance",
                                                "VGP.likelihood.scale", "VGP.q_mu", "VGP.q_sqrt"]
    gpx.set_trainable(m.likelihood.scale, False)
    assert [v.name for v in m.trainable_variables] == ["lengthscales:0", "variance:0", "q_mu:0", "q_sqrt:0"]
    g = _model(gpx.likelihoods.Gaussian(0.2))
    assert [v.name for v in g.trainable_variables] == ["lengthscales:0", "variance:0", "variance:0", "q_mu:0",
                                                       "q_sqrt:0"]
    assert g.trainable_variables[2]._param is g.likelihood.variance
    assert [n for n, _ in g._param_paths()][2] == "VGP.likelihood.variance"
    assert g.theta_row()[2] == pytest.approx(0.2)


def test_vgp_gradient_mapping_and_optimizer_dispatch():
    m = _model()
    n = 9
    rng = np.random.default_rng(0)
    gth = np.zeros(16)
    gth[:3] = [0.3, -1.2, 0.8]
    gq, gR = rng.standard_normal(n), np.tril(rng.standard_normal((n, n)))
    loss, gu = m.grads_to_unconstrained(m.trainable_variables, 2.5, gth, gq, gR)
    assert loss == -2.5 and gu.shape == (3 + n + n * (n + 1) // 2,)
    for i, p in enumerate((m.kernel.lengthscales, m.kernel.variance, m.likelihood.scale)):
        assert gu[i] == pytest.approx(-gth[i] * p.dtheta_du(), rel=1e-15)
    np.testing.assert_array_equal(gu[3:3 + n], -gq)
    # the q_sqrt block is the lower triangle in FillTriangular order: assigning it round-trips
    back = gpx.parameter.fill_triangular(-gu[3 + n:])
    np.testing.assert_array_equal(back, gR)
    from portfoliooptgp_amd.optimizers import _pack, _resolve_model, _unpack
    u = _pack(m.trainable_variables)
    assert u.shape == gu.shape
    _unpack(m.trainable_variables, u + 0.0)
    np.testing.assert_array_equal(_pack(m.trainable_variables), u)
    # the reference passes the bound method: Scipy().minimize(model.training_loss, ...)
    assert _resolve_model(m.training_loss) is m
    assert _resolve_model(m.training_loss_closure()) is m
    gpx.set_trainable(m.likelihood.scale, False)
    _, gu2 = m.grads_to_unconstrained(m.trainable_variables, 2.5, gth, gq, gR)
    np.testing.assert_array_equal(gu2, np.concatenate([gu[:2], gu[3:]]))


def test_vgp_refusals():
    X, Y = _data()
    k = gpx.kernels.SquaredExponential()
    st = gpx.likelihoods.StudentT()
    with pytest.raises(NotImplementedError):
        gpx.models.VGP((X, Y), k, st, mean_function=gpx.mean_functions.Constant())
    gpx.models.VGP((X, Y), k, st, mean_function=gpx.mean_functions.Zero())  # the zero mean is fine
    with pytest.raises(NotImplementedError):
        gpx.models.VGP((X, np.hstack([Y, Y])), k, st)
    with pytest.raises(NotImplementedError):
        gpx.models.VGP((X, Y), k, st, num_latent_gps=2)
    with pytest.raises(NotImplementedError):
        gpx.models.VGP((X, Y), k, object())
    with pytest.raises(ValueError):
        gpx.models.VGP((X, Y[:-1]), k, st)
    m = gpx.models.VGP((X, Y), k, st)
    for f in (m.predict_f, m.predict_y):
        with pytest.raises(NotImplementedError):
            f(X, full_cov=True)
        with pytest.raises(NotImplementedError):
            f(X, full_output_cov=True)
    # SVGP and SGPR keep refusing non-Gaussian likelihoods
    with pytest.raises(NotImplementedError):
        gpx.models.SVGP(kernel=k, likelihood=st, inducing_variable=X[:3])
    with pytest.raises(NotImplementedError):
        gpx.models.SGPR((X, Y), k, X[:3], likelihood=st)


def test_print_summary_lists_vgp_parameters(capsys):
    gpx.print_summary(_model())
    out = capsys.readouterr().out
    for name in ("VGP.kernel.lengthscales", "VGP.kernel.variance", "VGP.likelihood.scale", "VGP.q_mu",
                 "VGP.q_sqrt"):
        assert name in out, name
    assert "(9, 1)" in out and "(1, 9, 9)" in out and "FillTriangular" in out
    assert "df" not in out


def test_vgp_symbols_are_exported():
    for s in ("gpx_vgp_create", "gpx_vgp_destroy", "gpx_vgp_elbo_grad", "gpx_vgp_predict"):
        assert s in N.EXPORTED_SYMBOLS
    assert (N.GPX_LIK_GAUSSIAN, N.GPX_LIK_STUDENT_T) == (0, 1)
