"""The batched small-shape SGPR surface without a GPU: the limits query, what
Scipy().minimize_sgpr_batch refuses (before any device object exists), and the models
ModelTrainer.train_sgpr_model builds (the fit and the batched predict patched at their seams)."""
import ctypes

import numpy as np
import pytest
import torch

import portfoliooptgp_amd as gpx
from portfoliooptgp_amd import _native as N
from portfoliooptgp_amd import models as M
from portfoliooptgp_amd import optimizers
from portfoliooptgp_amd.engine import sgpr_small_limits
from portfoliooptgp_amd.trainer import ModelTrainer

K = gpx.kernels
SYMBOLS = ("gpx_sgpr_small_limits", "gpx_sgpr_small_create", "gpx_sgpr_small_bind", "gpx_sgpr_small_elbo_grad",
           "gpx_sgpr_small_predict", "gpx_sgpr_small_destroy")


def _xy(n=30, D=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 10, (n, D)), rng.standard_normal((n, 1))


def _sgpr(kernel=None, M_=5, D=1):
    return gpx.models.SGPR(_xy(D=D), kernel or K.SquaredExponential(),
                           inducing_variable=np.linspace(0, 10, M_)[:, None].repeat(D, 1))


def test_limits_need_no_device():
    lib = N.load_library()
    m, n = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.gpx_sgpr_small_limits(ctypes.byref(m), ctypes.byref(n)) == N.GPX_OK
    assert (m.value, n.value) == (32, 4096)
    assert sgpr_small_limits() == (32, 4096)
    assert lib.gpx_sgpr_small_limits(None, None) == N.GPX_BAD_ARG


def test_new_symbols_are_declared_and_bound():
    lib = N.load_library()
    for s in SYMBOLS:
        assert s in N.EXPORTED_SYMBOLS
        fn = getattr(lib, s)
        assert fn.restype is ctypes.c_int and fn.argtypes
    assert len(lib.gpx_sgpr_small_elbo_grad.argtypes) == 10
    assert len(lib.gpx_sgpr_small_predict.argtypes) == 11
    assert len(lib.gpx_sgpr_small_bind.argtypes) == 7


def test_null_handles_are_refused_without_a_device():
    lib = N.load_library()
    assert lib.gpx_sgpr_small_destroy(None) == N.GPX_BAD_ARG
    assert lib.gpx_sgpr_small_create(None, 1, 1, 1, 1, None) == N.GPX_BAD_ARG
    assert lib.gpx_sgpr_small_bind(None, 0, 1, 1, None, None, None) == N.GPX_BAD_ARG
    assert lib.gpx_sgpr_small_elbo_grad(None, 0, None, None, None, None, None, None, None, None) == N.GPX_BAD_ARG
    assert lib.gpx_sgpr_small_predict(None, 0, None, None, None, 0, 0, None, None, None, None) == N.GPX_BAD_ARG


def test_mixed_input_dimension_is_refused():
    with pytest.raises(ValueError, match=r"share the input dimension D, got \[1, 2\]"):
        gpx.optimizers.Scipy().minimize_sgpr_batch([_sgpr(), _sgpr(D=2)])


def test_bad_policy_other_methods_and_non_sgpr_models():
    x, y = _xy()
    opt = gpx.optimizers.Scipy()
    with pytest.raises(ValueError, match="on_not_pd"):
        opt.minimize_sgpr_batch([_sgpr()], on_not_pd="ignore")
    with pytest.raises(NotImplementedError, match="L-BFGS-B"):
        opt.minimize_sgpr_batch([_sgpr()], method="BFGS")
    with pytest.raises(NotImplementedError, match="L-BFGS-B"):
        opt.minimize_sgpr_batch([_sgpr()], bounds=[(0, 1)])
    with pytest.raises(TypeError, match="model 1 is not a models.SGPR"):
        opt.minimize_sgpr_batch([_sgpr(), gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential())])
    with pytest.raises(TypeError, match="not a models.SGPR"):
        opt.minimize_sgpr_batch([gpx.models.SVGP(kernel=K.SquaredExponential(),
                                                 likelihood=gpx.likelihoods.Gaussian(),
                                                 inducing_variable=np.zeros((3, 1)))])
    assert opt.minimize_sgpr_batch([]) == []


def test_predict_batch_of_nothing_is_empty():
    assert M.predict_f_sgpr_batch([], []) == []


@pytest.mark.parametrize("n,D,n_inducing", [(113, 1, 10), (5, 1, 10), (40, 3, 7)])
def test_train_sgpr_model_builds_the_reference_models(monkeypatch, n, D, n_inducing):
    """One SGPR per kernel with GPflow's defaults (noise 1.0 trainable, Z trainable), Z0 the linspace
    grid over X's range for D = 1 and evenly spaced rows of X otherwise; one minimize_sgpr_batch with
    maxiter, one batched predict at X, strict-< MSE choice."""
    rng = np.random.default_rng(1)
    x = np.sort(rng.uniform(3, 360, (n, D)), axis=0)
    y = np.sin(x[:, :1] / 7.0)
    seen = {}

    def fake_fit(self, models, method="L-BFGS-B", on_not_pd="raise", **kw):
        seen["models"], seen["kw"] = list(models), kw
        return ["res%d" % i for i in range(len(models))]

    def fake_predict(models, Xnews, add_noise=False):
        seen["Xnews"] = list(Xnews)
        # model 3 predicts exactly, models 3 and 5 tie: the first of the best wins
        return [(torch.as_tensor(y) + (0.0 if i in (3, 5) else 0.1 * (i + 1)), torch.ones(n, 1))
                for i in range(len(models))]

    monkeypatch.setattr(optimizers.Scipy, "minimize_sgpr_batch", fake_fit)
    monkeypatch.setattr(M, "predict_f_sgpr_batch", fake_predict)
    ks = [K.SquaredExponential(), K.Matern12(), K.RationalQuadratic(), K.Exponential(),
          K.SquaredExponential() + K.Matern12(), K.Exponential() + K.Periodic(K.SquaredExponential()) + K.Linear(),
          K.Exponential() + K.Periodic(K.SquaredExponential()), K.SquaredExponential() * K.Matern12()]
    tr = ModelTrainer(ks)
    best_kernel, best_mse, best_model = tr.train_sgpr_model(x, y, n_inducing=n_inducing, maxiter=37)
    ms = seen["models"]
    assert len(ms) == 8 and tr.last_models == ms and tr.last_results == ["res%d" % i for i in range(8)]
    assert seen["kw"] == dict(options=dict(maxiter=37))
    assert len(seen["Xnews"]) == 8 and all(xn is x for xn in seen["Xnews"])
    if D == 1:
        z0 = np.linspace(x.min(), x.max(), n_inducing)[:, None]
    else:
        z0 = x[np.linspace(0, n - 1, n_inducing).round().astype(int)]
    for m, k in zip(ms, ks):
        assert isinstance(m, gpx.models.SGPR) and m.kernel is k
        assert m.M == n_inducing
        np.testing.assert_array_equal(m.inducing_variable.Z.value, z0)
        np.testing.assert_array_equal(m.data[0].numpy(), x)
        assert isinstance(m.likelihood, gpx.likelihoods.Gaussian) and m.likelihood.variance.value == pytest.approx(1.0)
        assert m.likelihood.variance.trainable and m.inducing_variable.Z.trainable
        assert len(m.trainable_variables) == 2 + len(k.parameters)  # Z, the kernel's, the noise variance
    assert best_kernel is ks[3] and best_model is ms[3] and best_mse == 0.0
    # the models own their inducing points: one model's Z is not another's
    ms[0].inducing_variable.Z.assign(ms[0].inducing_variable.Z.value + 1.0)
    np.testing.assert_array_equal(ms[1].inducing_variable.Z.value, z0)
