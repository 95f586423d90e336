"""Batched small-shape SVGP on the GPU (libgpx.so gpx_svgp_small_*, engine.SVGPSmallEngine,
Scipy().minimize_svgp_batch, models.predict_f_svgp_batch, ModelTrainer.train_svgp_model) against the
SVGP oracle (oracle/svgp_oracle.py) and against the existing one-model path.

Inputs: tests/svgp_batch_cases.py (thirteen cases; cond(Kmm + 1e-6 I) <= 1e4 is asserted, so an
ill-conditioned input cannot pass as well-conditioned). A gpx_svgp_small object has ONE input
dimension, so the thirteen cases make three calls: the ten D = 1 cases in one, the two D = 2 cases in
one, the D = 3 case alone; "the full call" below is a case's D group.

Tolerances are tests/test_svgp_gpu.py's for this model (fp64):
  ELBO          |Δ| <= 1e-9 · |ref|
  gradients     max|Δ| <= 1e-7 · (1 + max|g_ref|) per block (θ, noise, Z, q_mu, q_sqrt)
  predictions   max|Δ| <= 1e-7 · max|ref| + 1e-10
  fitted loss   1e-6 relative to the existing path after 8 L-BFGS-B iterations (the bar of
                test_scipy_fit_tracks_oracle_fit, for its reason: the iterations amplify evaluation rounding)
  fitted MSE    1e-5 relative (SURVEY §8c's bar for fitted quantities)
Everything "bit for bit" is compared with == / assert_array_equal."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import portfoliooptgp_amd as gpx  # noqa: E402
from portfoliooptgp_amd import _native as N  # noqa: E402
from portfoliooptgp_amd.engine import SVGPSmallEngine  # noqa: E402
from portfoliooptgp_amd.kernels import compile_spec  # noqa: E402
from portfoliooptgp_amd.trainer import ModelTrainer, mean_squared_error  # noqa: E402
from oracle import svgp_oracle as S  # noqa: E402
from tests import svgp_batch_cases as C  # noqa: E402
from tests.test_callers_gpu import ref_kernels  # noqa: E402
from tests.test_svgp_gpu import _check  # noqa: E402

N_MAX, M_MAX = 1024, 32  # above every case's own size (M = 32 is the path's limit and one case's size)


def _theta(gk, noise):
    row = np.ones(N.GPX_THETA_STRIDE)
    kp = gk.parameters
    for i, p in enumerate(kp):
        row[i] = p.value
    row[len(kp)] = noise
    return row


@pytest.fixture(scope="module")
def cases():
    return [C.make_case(i) for i in range(len(C.CASES))]


def _groups(cases):
    g = {}
    for i, c in enumerate(cases):
        g.setdefault(c["D"], []).append(i)
    return g


def _engine(cases, idx, nan_tails=False, B=None, n_max=N_MAX, m_max=M_MAX):
    """An engine holding cases idx in slots 0..; nan_tails: every slot's X / Y tail and the tails of
    its Z / q_mu / q_sqrt rows are NaN."""
    D = cases[idx[0]]["D"]
    eng = SVGPSmallEngine(B or len(idx), n_max, m_max, D)
    for s, i in enumerate(idx):
        c = cases[i]
        spec = compile_spec(c["gk"], D)
        if nan_tails:
            eng.bind(s, np.full((n_max, D), np.nan), np.full(n_max, np.nan), spec, 1)
            eng.Z[s], eng.q_mu[s], eng.q_sqrt[s] = np.nan, np.nan, np.nan
        eng.bind(s, c["X"], c["Y"], spec, c["M"], num_data=c["n"])
        eng.pack(s, _theta(c["gk"], c["noise"]), c["Z"], c["q"], c["R"])
    return eng


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)


@pytest.fixture(scope="module")
def full(cases):
    """{case: outputs} from the full call of its D group (all slots active, in order)."""
    out = {}
    for D, idx in _groups(cases).items():
        eng = _engine(cases, idx)
        info = eng.elbo_grad(list(range(len(idx))))
        assert not info[:len(idx)].any(), info
        for s, i in enumerate(idx):
            out[i] = eng.result(s)
    return out


def test_inputs_are_well_conditioned(cases):
    for i, c in enumerate(cases):
        assert C.cond_kmm(c) <= C.COND_CAP, (i, C.CASES[i], C.cond_kmm(c))


def test_elbo_and_gradients_vs_oracle(cases, full):
    for i, c in enumerate(cases):
        assert C.cond_kmm(c) <= C.COND_CAP
        om = S.OSVGP(c["ok"], c["Z"], num_data=c["n"], noise_variance=c["noise"], q_mu=c["q"], q_sqrt=c["R"])
        ref = om.elbo_and_grads(c["X"], c["Y"])
        got = full[i]
        print(C.CASES[i], "ELBO", got[0], ref[0], "rel", abs(got[0] - ref[0]) / abs(ref[0]))
        _check(got, ref, (1e-9, 1e-7))


def test_composition_invariance_bitwise(cases, full):
    """A model's outputs from the full call == from a call holding it alone (another object, B = 1,
    its own N_max / M_max) == from the full call with the active list reversed."""
    for D, idx in _groups(cases).items():
        eng = _engine(cases, idx)
        eng.elbo_grad(list(range(len(idx)))[::-1])
        for s, i in enumerate(idx):
            _same(eng.result(s), full[i])
        eng.elbo_grad([len(idx) - 1])  # one slot of the shared object alone
        _same(eng.result(len(idx) - 1), full[idx[-1]])
    for i, c in enumerate(cases):
        solo = _engine(cases, [i], n_max=c["n"], m_max=c["M"])
        solo.elbo_grad([0])
        _same(solo.result(0), full[i])


def test_tails_are_not_read(cases, full):
    for D, idx in _groups(cases).items():
        eng = _engine(cases, idx, nan_tails=True)
        info = eng.elbo_grad(list(range(len(idx))))
        assert not info[:len(idx)].any()
        for s, i in enumerate(idx):
            _same(eng.result(s), full[i])


def test_predict_vs_oracle(cases):
    rng = np.random.default_rng(8)
    for i, xs in ((8, rng.uniform(-1, 11, (333, 2))), (0, cases[0]["X"])):
        c = cases[i]
        eng = _engine(cases, [i])
        om = S.OSVGP(c["ok"], c["Z"], num_data=c["n"], noise_variance=c["noise"], q_mu=c["q"], q_sqrt=c["R"])
        th = _theta(c["gk"], c["noise"])
        for add_noise, (mo, vo) in ((False, om.predict_f(xs)), (True, om.predict_y(xs))):
            mu, var = eng.predict(0, th, c["Z"], c["q"], c["R"], xs, add_noise)
            em, ev = np.abs(mu - mo[:, 0]).max(), np.abs(var - vo[:, 0]).max()
            print(C.CASES[i], "predict_y" if add_noise else "predict_f", em, ev)
            assert em <= 1e-7 * np.abs(mo).max() + 1e-10
            assert ev <= 1e-7 * np.abs(vo).max() + 1e-10
        mu0, var0 = eng.predict(0, th, c["Z"], c["q"], c["R"], np.zeros((0, c["D"])), False)
        assert mu0.shape == (0,) and var0.shape == (0,)


# ---- fits -----------------------------------------------------------------------------------------

def _days():
    """The days layout at n = 89: X = arange(89), Y z-scored normal draws. Seed 0 was picked on the
    CPU oracle: over the 8 kernels' maxiter = 8 fits no hyperparameter leaves [1.9e-4, 4] (other
    seeds drive the Periodic fit's softplus to 0 or overflow), and the best training MSE is 1.8 %
    below the runner-up."""
    return C.days_xy(89, 0)


def _model(kernel, x, m=20, noise=1e-4):
    sv = gpx.models.SVGP(kernel=kernel, likelihood=gpx.likelihoods.Gaussian(variance=noise),
                         inducing_variable=x[:m].copy())
    gpx.set_trainable(sv.likelihood.variance, False)
    return sv


def _same_result(a, b):
    np.testing.assert_array_equal(a.x, b.x)
    assert (a.fun, a.nit, a.nfev) == (b.fun, b.nit, b.nfev), ((a.fun, a.nit, a.nfev), (b.fun, b.nit, b.nfev))


OPTS = dict(maxiter=8)


def test_batch_fit_equals_solo_fit_and_tracks_existing_path():
    x, y = _days()
    opt = gpx.optimizers.Scipy()
    batch = opt.minimize_svgp_batch([_model(k, x) for k in ref_kernels()], (x, y), options=OPTS)
    for i, k in enumerate(ref_kernels()):
        alone = opt.minimize_svgp_batch([_model(k, x)], (x, y), options=OPTS)[0]
        _same_result(batch[i], alone)
    for i, k in enumerate(ref_kernels()):
        m = _model(k, x)
        ref = opt.minimize(m.training_loss_closure((x, y)), m.trainable_variables, options=OPTS)
        print(i, "fun", batch[i].fun, ref.fun, "rel", abs(batch[i].fun - ref.fun) / abs(ref.fun))
        assert batch[i].fun == pytest.approx(ref.fun, rel=1e-6)


def test_per_model_data_and_written_back_state():
    """One (X, Y) pair per model (different n), and the fitted values are in the models."""
    x, y = _days()
    ks = ref_kernels()[:3]
    ms = [_model(k, x[:n], m=10) for k, n in zip(ks, (89, 40, 11))]
    res = gpx.optimizers.Scipy().minimize_svgp_batch(ms, [(x[:n], y[:n]) for n in (89, 40, 11)], options=OPTS)
    for m, r, n in zip(ms, res, (89, 40, 11)):
        alone = _model(type(m.kernel)(), x[:n], m=10)
        ra = gpx.optimizers.Scipy().minimize_svgp_batch([alone], (x[:n], y[:n]), options=OPTS)[0]
        _same_result(r, ra)
        np.testing.assert_array_equal(m.q_sqrt.value, alone.q_sqrt.value)
        np.testing.assert_array_equal(m.inducing_variable.Z.value, alone.inducing_variable.Z.value)


def test_over_limit_model_takes_the_existing_path():
    x, y = _days()
    K = gpx.kernels
    opt = gpx.optimizers.Scipy()
    mk = lambda: [_model(K.SquaredExponential(), x), _model(K.Matern12(), x, m=40), _model(K.Matern32(), x, m=7)]  # noqa: E731
    ms = mk()
    res = opt.minimize_svgp_batch(ms, (x, y), options=OPTS)
    ref = mk()
    r1 = opt.minimize(ref[1].training_loss_closure((x, y)), ref[1].trainable_variables, options=OPTS)
    _same_result(res[1], r1)
    for i in (0, 2):
        _same_result(res[i], opt.minimize_svgp_batch([ref[i]], (x, y), options=OPTS)[0])
    # prediction: the bound slots, and the over-limit model by its own engine
    preds = gpx.models.predict_f_svgp_batch(ms, [x, x, x])
    m1, v1 = ref[1].predict_f(x)
    np.testing.assert_array_equal(preds[1][0].numpy(), m1.numpy())
    for (mu, var), m in zip(preds, ms):
        assert tuple(mu.shape) == (89, 1) and tuple(var.shape) == (89, 1)
    mu0, var0 = gpx.models.predict_f_svgp_batch(ms[:1], [np.zeros((0, 1))])[0]
    assert tuple(mu0.shape) == (0, 1) and tuple(var0.shape) == (0, 1)


def _not_pd_models(x):
    K = gpx.kernels
    bad = _model(K.SquaredExponential(variance=2.0 ** 40), x)
    z = bad.inducing_variable.Z.value.copy()
    z[1] = z[0]  # two identical inducing rows: the second pivot of Kmm + 1e-6 I is exactly 0
    bad.inducing_variable.Z.assign(z)
    return [_model(K.Matern32(), x), bad, _model(K.Exponential(), x)]


def test_not_pd_raises_by_default_and_inf_keeps_the_others():
    x, y = _days()
    opt = gpx.optimizers.Scipy()
    solo = _not_pd_models(x)[1]
    with pytest.raises(gpx.NotPositiveDefiniteError):
        opt.minimize(solo.training_loss_closure((x, y)), solo.trainable_variables, options=OPTS)
    with pytest.raises(gpx.NotPositiveDefiniteError):
        opt.minimize_svgp_batch(_not_pd_models(x), (x, y), options=OPTS)
    ms = _not_pd_models(x)
    res = opt.minimize_svgp_batch(ms, (x, y), options=OPTS, on_not_pd="inf")
    assert len(res) == 3 and res[1].fun == float("inf")
    ref = _not_pd_models(x)
    for i in (0, 2):
        _same_result(res[i], opt.minimize_svgp_batch([ref[i]], (x, y), options=OPTS)[0])


def test_train_svgp_model_matches_the_loop_of_solo_fits():
    x, y = _days()
    opt = gpx.optimizers.Scipy()
    solo_mse = []
    for k in ref_kernels():
        m = _model(k, x)
        opt.minimize(m.training_loss_closure((x, y)), m.trainable_variables, options=OPTS)
        solo_mse.append(mean_squared_error(y, m.predict_f(x)[0].numpy()))
    s = sorted(solo_mse)
    print("solo MSE", solo_mse)
    assert (s[1] - s[0]) / s[0] > 1e-3, solo_mse  # the winner is not decided by a tie
    ks = ref_kernels()
    tr = ModelTrainer(ks)
    best_kernel, best_mse, best_model = tr.train_svgp_model(x, y, n_inducing=20, maxiter=8)
    mses = [mean_squared_error(y, p[0].numpy())
            for p in gpx.models.predict_f_svgp_batch(tr.last_models, [x] * len(ks))]
    print("batch MSE", mses)
    for a, b in zip(mses, solo_mse):
        assert a == pytest.approx(b, rel=1e-5)
    assert best_kernel is ks[int(np.argmin(solo_mse))]
    assert best_mse == min(mses) and best_model is tr.last_models[int(np.argmin(solo_mse))]
