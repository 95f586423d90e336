"""Posterior sampling without a GPU: the C symbols, the refusals that happen before any device call
(as tests/test_ard_api.py checks construction-time refusals), and the numpy restatement's own error
(tests/sample_numpy.py: its two Cholesky routes against each other and against Higham's bound)."""
import ctypes

import numpy as np
import pytest

import portfoliooptgp_amd as gpx
from portfoliooptgp_amd import _native as N
from portfoliooptgp_amd import engine, trainer
from tests import sample_numpy as SN

K = gpx.kernels


def _gpr():
    x = np.arange(7, dtype=np.float64)[:, None]
    return gpx.models.GPR((x, np.sin(x)), kernel=K.SquaredExponential(), noise_variance=1e-2)


# ------------------------------------------------------------------------------------- C ABI
def test_symbols_and_limits_without_a_device():
    lib = N.load_library()
    for sym in ("gpx_sample_limits", "gpx_sample_mvn", "gpx_batch_predict_samples"):
        assert sym in N.EXPORTED_SYMBOLS and hasattr(lib, sym), sym
    m = ctypes.c_int(0)
    assert lib.gpx_sample_limits(ctypes.byref(m)) == N.GPX_OK
    assert m.value >= 1024 and engine.sample_limits() == m.value
    assert lib.gpx_sample_limits(None) == N.GPX_BAD_ARG


def test_null_handles_are_bad_arg_without_a_device():
    lib = N.load_library()
    buf = (ctypes.c_double * 4)()
    info = (ctypes.c_int32 * 1)()
    act = (ctypes.c_int32 * 1)(0)
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gpx_sample_mvn(None, 1, 1, 1, p, p, p, 1e-6, p, info, None) == N.GPX_BAD_ARG
    assert lib.gpx_batch_predict_samples(None, 1, act, buf, p, 1, 1, p, 1e-6, p, p, info, None) == N.GPX_BAD_ARG


# ------------------------------------------------------------------------ refusals before the device
def test_predict_f_samples_refuses_bad_arguments_before_any_device_call():
    m = _gpr()
    xs = np.linspace(0, 3, 4)[:, None]
    for bad in (0, -3):
        with pytest.raises(ValueError, match="num_samples"):
            m.predict_f_samples(xs, bad)
    with pytest.raises(ValueError, match="white"):
        m.predict_f_samples(xs, 2, white=np.zeros((2, 5, 1)))
    with pytest.raises(ValueError, match="white"):
        m.predict_f_samples(xs, white=np.zeros((1, 4, 1)))   # no num_samples: [N*, 1]
    with pytest.raises(NotImplementedError, match="full_output_cov"):
        m.predict_f_samples(xs, 2, full_cov=True, full_output_cov=True)
    with pytest.raises(ValueError, match="jitter"):
        m.predict_f_samples(xs, 2, jitter=-1e-6)
    with pytest.raises(ValueError, match="jitter"):
        m.predict_f_samples(xs, 2, jitter=float("nan"))
    with pytest.raises(ValueError, match="num_samples"):
        gpx.models.predict_f_samples_batch([m], [xs], 0)
    assert m._engine is None   # nothing reached the device


def test_predict_log_density_with_student_t_raises():
    x = np.linspace(0, 5, 12)[:, None]
    y = np.sin(x)
    vg = gpx.models.VGP((x, y), kernel=K.SquaredExponential(), likelihood=gpx.likelihoods.StudentT())
    with pytest.raises(NotImplementedError, match="Gaussian"):
        vg.predict_log_density((x, y))
    sv = gpx.models.SVGP(kernel=K.SquaredExponential(), likelihood=gpx.likelihoods.StudentT(),
                         inducing_variable=x[:4], num_data=12, per_point=True)
    with pytest.raises(NotImplementedError, match="Gaussian"):
        sv.predict_log_density((x, y))


def test_sample_asset_paths_refuses_ragged_assets():
    xa = np.array([[0.0, 0], [1.0, 0], [0.0, 1]])   # asset 0: two rows, asset 1: one

    class Never:
        def predict_f_samples(self, *a, **k):
            raise AssertionError("reached the model")
    with pytest.raises(ValueError, match="same number of rows"):
        trainer.sample_asset_paths(Never(), xa, 1, 4)


# ----------------------------------------------------------------------------- the restatement
@pytest.mark.parametrize("name", ["se", "m52"])
def test_restatement_routes_agree_and_meet_the_factor_bound(name):
    """LAPACK's factor and the unblocked column Cholesky on cov + 1e-6·I of the SE (ℓ = 5, noise
    1e-5) and Matern52 (ℓ = 3, noise 1e-3) posteriors at every M of the GPU test: the residual of
    each within (M+1)·u·sqrt(A_ii A_jj), the draws of the two within the perturbation bound."""
    om = SN.se_oracle() if name == "se" else SN.matern_oracle()
    rng = np.random.default_rng(5)
    for M in SN.MS:
        mean, cov = om.predict_f(SN.xs_for(M), full_cov=True)
        A = cov + SN.JITTER * np.eye(M)
        assert np.linalg.cond(A) <= 2.5e7
        bound = SN.factor_bound(A)
        for chol in (SN.chol_lapack, SN.chol_columns):
            L = chol(A)
            assert np.all(np.abs(L @ L.T - A) <= bound), (name, M, chol.__name__)
        white = rng.standard_normal((3, M))
        a = SN.sample_mvn(mean[:, 0], cov, white, chol=SN.chol_lapack)
        b = SN.sample_mvn(mean[:, 0], cov, white, chol=SN.chol_columns)
        assert np.all(np.abs(a - b).max(axis=1) <= SN.sample_bound(A, SN.chol_lapack(A), white)), (name, M)


def test_column_cholesky_reports_the_first_bad_pivot():
    A = np.eye(17)
    A[0, 1] = A[1, 0] = 2.0
    with pytest.raises(np.linalg.LinAlgError, match="pivot 2"):
        SN.chol_columns(A)
