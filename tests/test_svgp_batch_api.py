"""The batched small-shape SVGP surface without a GPU: the limits query, what
Scipy().minimize_svgp_batch refuses (before any device object exists), and the models
ModelTrainer.train_svgp_model builds (the fit and the batched predict patched at their seams)."""
import ctypes

import numpy as np
import pytest
import torch

import portfoliooptgp_amd as gpx
from portfoliooptgp_amd import _native as N
from portfoliooptgp_amd import models as M
from portfoliooptgp_amd import optimizers
from portfoliooptgp_amd.engine import svgp_small_limits
from portfoliooptgp_amd.trainer import ModelTrainer

K = gpx.kernels


def _xy(n=30, D=1, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(0, 10, (n, D)), rng.standard_normal((n, 1))


def _svgp(kernel=None, M_=5, D=1, **kw):
    lik = kw.pop("likelihood", None) or gpx.likelihoods.Gaussian(variance=1e-4)
    return gpx.models.SVGP(kernel=kernel or K.SquaredExponential(), likelihood=lik,
                           inducing_variable=np.linspace(0, 10, M_)[:, None].repeat(D, 1), **kw)


def test_limits_need_no_device():
    lib = N.load_library()
    m, n = ctypes.c_int(0), ctypes.c_int(0)
    assert lib.gpx_svgp_small_limits(ctypes.byref(m), ctypes.byref(n)) == N.GPX_OK
    assert (m.value, n.value) == (32, 4096)
    assert svgp_small_limits() == (32, 4096)
    assert lib.gpx_svgp_small_limits(None, None) == N.GPX_BAD_ARG


def test_new_symbols_are_declared():
    for s in ("gpx_svgp_small_limits", "gpx_svgp_small_create", "gpx_svgp_small_bind", "gpx_svgp_small_elbo_grad",
              "gpx_svgp_small_predict", "gpx_svgp_small_destroy"):
        assert s in N.EXPORTED_SYMBOLS


def test_student_t_is_refused_with_its_reason():
    x, y = _xy()
    st = _svgp(likelihood=gpx.likelihoods.StudentT(), per_point=True)
    with pytest.raises(NotImplementedError, match="StudentT likelihood"):
        gpx.optimizers.Scipy().minimize_svgp_batch([_svgp(), st], (x, y))


def test_per_point_is_refused_with_its_reason():
    x, y = _xy()
    with pytest.raises(NotImplementedError, match="per_point=True"):
        gpx.optimizers.Scipy().minimize_svgp_batch([_svgp(per_point=True)], (x, y))


def test_mixed_input_dimension_is_refused():
    (x1, y1), (x2, y2) = _xy(D=1), _xy(D=2)
    with pytest.raises(ValueError, match=r"share the input dimension D, got \[1, 2\]"):
        gpx.optimizers.Scipy().minimize_svgp_batch([_svgp(), _svgp(D=2)], [(x1, y1), (x2, y2)])


def test_data_must_be_one_pair_or_one_per_model():
    x, y = _xy()
    with pytest.raises(ValueError, match="one pair per model"):
        gpx.optimizers.Scipy().minimize_svgp_batch([_svgp(), _svgp()], [(x, y)])


def test_bad_policy_other_methods_and_non_svgp_models():
    x, y = _xy()
    opt = gpx.optimizers.Scipy()
    with pytest.raises(ValueError, match="on_not_pd"):
        opt.minimize_svgp_batch([_svgp()], (x, y), on_not_pd="ignore")
    with pytest.raises(NotImplementedError, match="L-BFGS-B"):
        opt.minimize_svgp_batch([_svgp()], (x, y), method="BFGS")
    with pytest.raises(TypeError, match="not a models.SVGP"):
        opt.minimize_svgp_batch([gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential())], (x, y))
    assert opt.minimize_svgp_batch([], (x, y)) == []


@pytest.mark.parametrize("n,n_inducing", [(89, 20), (5, 20), (19, 7)])
def test_train_svgp_model_builds_the_reference_models(monkeypatch, n, n_inducing):
    """8 models, M = min(n_inducing, N), Z = the first rows, Gaussian(1e-4) frozen, num_data None; one
    minimize_svgp_batch over (X, Y) with maxiter, one batched predict at X, strict-< MSE choice."""
    x = np.arange(n, dtype=np.float64)[:, None]
    y = np.sin(x / 7.0)
    seen = {}

    def fake_fit(self, models, data, method="L-BFGS-B", on_not_pd="raise", **kw):
        seen["models"], seen["data"], seen["kw"] = list(models), data, kw
        return ["res%d" % i for i in range(len(models))]

    def fake_predict(models, Xnews, add_noise=False):
        seen["Xnews"] = list(Xnews)
        # model 3 predicts exactly, models 3 and 5 tie: the first of the best wins
        return [(torch.as_tensor(y) + (0.0 if i in (3, 5) else 0.1 * (i + 1)), torch.ones(n, 1))
                for i in range(len(models))]

    monkeypatch.setattr(optimizers.Scipy, "minimize_svgp_batch", fake_fit)
    monkeypatch.setattr(M, "predict_f_svgp_batch", fake_predict)
    ks = [K.SquaredExponential(), K.Matern12(), K.RationalQuadratic(), K.Exponential(),
          K.SquaredExponential() + K.Matern12(), K.Exponential() + K.Periodic(K.SquaredExponential()) + K.Linear(),
          K.Exponential() + K.Periodic(K.SquaredExponential()), K.SquaredExponential() * K.Matern12()]
    tr = ModelTrainer(ks)
    best_kernel, best_mse, best_model = tr.train_svgp_model(x, y, n_inducing=n_inducing, maxiter=37)
    ms = seen["models"]
    assert len(ms) == 8 and tr.last_models == ms and tr.last_results == ["res%d" % i for i in range(8)]
    assert seen["data"][0] is x and seen["data"][1] is y and seen["kw"] == dict(options=dict(maxiter=37))
    assert len(seen["Xnews"]) == 8 and all(xn is x for xn in seen["Xnews"])
    for m, k in zip(ms, ks):
        assert isinstance(m, gpx.models.SVGP) and m.kernel is k
        assert m.M == min(n_inducing, n)
        np.testing.assert_array_equal(m.inducing_variable.Z.value, x[:n_inducing])
        assert isinstance(m.likelihood, gpx.likelihoods.Gaussian) and m.likelihood.variance.value == pytest.approx(1e-4)
        assert not m.likelihood.variance.trainable and m.num_data is None and not m.per_point
        assert len(m.trainable_variables) == 3 + len(k.parameters)  # Z, the kernel's, q_mu, q_sqrt
    assert best_kernel is ks[3] and best_model is ms[3] and best_mse == 0.0
    # the models own their inducing points: one model's Z is not another's
    ms[0].inducing_variable.Z.assign(ms[0].inducing_variable.Z.value + 1.0)
    np.testing.assert_array_equal(ms[1].inducing_variable.Z.value, x[:n_inducing])
