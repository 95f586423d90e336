"""SGPR model surface on the CPU (no device calls): GPflow variable order and shapes, the
constrained → unconstrained gradient mapping against the restatement (tests/sgpr_numpy.py), what
the model refuses, and print_summary."""
import numpy as np
import pytest
import torch

import portfoliooptgp_amd as gpx
from oracle import gp_oracle as O
from tests.sgpr_numpy import NumpySGPR


def _data(n=40, seed=3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, 1))
    return X, np.sin(X) + 0.1 * rng.standard_normal((n, 1))


def _model(M=5, **kw):
    X, Y = _data()
    k = gpx.kernels.SquaredExponential(lengthscales=1.5, variance=0.7)
    return gpx.models.SGPR((X, Y), kernel=k, inducing_variable=np.linspace(0, 10, M)[:, None], **kw)


def test_sgpr_is_exported_with_gpflow_attributes():
    m = _model()
    assert gpx.models.SGPR is type(m)
    assert m.num_latent_gps == 1
    assert isinstance(m.likelihood, gpx.likelihoods.Gaussian)
    assert m.likelihood.variance.value == pytest.approx(1.0)  # GPflow's default noise_variance
    assert isinstance(m.inducing_variable, gpx.inducing_variables.InducingPoints)
    assert tuple(m.data[0].shape) == (40, 1) and tuple(m.data[1].shape) == (40, 1)
    assert m.data[0].dtype == torch.float64
    assert _model(noise_variance=0.25).likelihood.variance.value == pytest.approx(0.25)
    assert _model(likelihood=gpx.likelihoods.Gaussian(0.5)).likelihood.variance.value == pytest.approx(0.5)
    for name in ("elbo", "maximum_log_likelihood_objective", "training_loss", "training_loss_closure",
                 "loss_and_grad_unconstrained", "predict_f", "predict_y"):
        assert callable(getattr(m, name))


def test_sgpr_variables_follow_gpflow_order_and_shapes():
    m = _model()
    names = [v.name for v in m.trainable_variables]
    assert names == ["Z:0", "lengthscales:0", "variance:0", "variance:0"]
    assert [tuple(v.shape) for v in m.trainable_variables] == [(5, 1), (), (), ()]
    assert m.trainable_variables[3]._param is m.likelihood.variance
    gpx.set_trainable(m.likelihood.variance, False)
    assert [v.name for v in m.trainable_variables] == ["Z:0", "lengthscales:0", "variance:0"]
    gpx.set_trainable(m.inducing_variable.Z, False)
    assert [v.name for v in m.trainable_variables] == ["lengthscales:0", "variance:0"]


def test_sgpr_gradient_mapping_matches_restatement():
    m = _model(noise_variance=0.3)
    X, Y = _data()
    om = NumpySGPR(O.OSquaredExponential(lengthscales=1.5, variance=0.7), X, Y,
                   m.inducing_variable.Z.value, noise_variance=0.3)
    lo, go = om.loss_and_grad_u()
    F, g = om.elbo_and_grads()
    gth = np.zeros(16)
    gth[:2] = g["theta"]
    gth[2] = g["noise"]
    loss, gu = m.grads_to_unconstrained(m.trainable_variables, F, gth, g["Z"])
    assert loss == pytest.approx(lo, rel=1e-15)
    np.testing.assert_allclose(gu, go, rtol=1e-14, atol=1e-14)
    from portfoliooptgp_amd.optimizers import _pack, _resolve_model, _unpack
    u = _pack(m.trainable_variables)
    np.testing.assert_allclose(u, om.get_u(), rtol=1e-15)
    _unpack(m.trainable_variables, u + 0.0)
    np.testing.assert_array_equal(_pack(m.trainable_variables), u)
    # the reference passes the bound method: Scipy().minimize(model.training_loss, ...)
    assert _resolve_model(m.training_loss) is m
    assert _resolve_model(m.training_loss_closure()) is m
    # frozen noise (the other reference protocol) drops its column
    gpx.set_trainable(m.likelihood.variance, False)
    om.noise.trainable = False
    _, gu = m.grads_to_unconstrained(m.trainable_variables, F, gth, g["Z"])
    np.testing.assert_allclose(gu, om.loss_and_grad_u()[1], rtol=1e-14, atol=1e-14)


def test_sgpr_refusals():
    X, Y = _data()
    k = gpx.kernels.SquaredExponential()
    Z = np.linspace(0, 10, 4)[:, None]
    with pytest.raises(NotImplementedError):
        gpx.models.SGPR((X, Y), k, Z, mean_function=gpx.mean_functions.Constant())
    gpx.models.SGPR((X, Y), k, Z, mean_function=gpx.mean_functions.Zero())  # the zero mean is fine
    with pytest.raises(NotImplementedError):
        gpx.models.SGPR((X, np.hstack([Y, Y])), k, Z)
    with pytest.raises(NotImplementedError):
        gpx.models.SGPR((X, Y), k, Z, num_latent_gps=2)
    with pytest.raises(NotImplementedError):
        gpx.models.SGPR((X, Y), k, Z, likelihood=object())
    with pytest.raises(ValueError):
        gpx.models.SGPR((X, Y), k, Z, noise_variance=0.1, likelihood=gpx.likelihoods.Gaussian(0.1))
    with pytest.raises(ValueError):
        gpx.models.SGPR((X, Y), k, np.zeros((4, 2)))
    m = gpx.models.SGPR((X, Y), k, Z)
    for f in (m.predict_f, m.predict_y):
        with pytest.raises(NotImplementedError):
            f(X, full_cov=True)
        with pytest.raises(NotImplementedError):
            f(X, full_output_cov=True)


def test_print_summary_lists_sgpr_parameters(capsys):
    gpx.print_summary(_model())
    out = capsys.readouterr().out
    for name in ("SGPR.inducing_variable.Z", "SGPR.kernel.lengthscales", "SGPR.kernel.variance",
                 "SGPR.likelihood.variance"):
        assert name in out, name
    assert "(5, 1)" in out
