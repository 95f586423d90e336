"""Batched small-shape SGPR on the GPU (libgpx.so gpx_sgpr_small_*, engine.SGPRSmallEngine,
Scipy().minimize_sgpr_batch, models.predict_f_sgpr_batch, ModelTrainer.train_sgpr_model) against the
CPU restatement (tests/sgpr_numpy.NumpySGPR) and against the existing one-model path.

Inputs: tests/sgpr_batch_cases.py (twelve cases; cond(Kmm) <= 1e5 is asserted, so an ill-conditioned
input cannot hide behind a loose bar). A gpx_sgpr_small object has ONE input dimension, so the cases
make four calls (D = 1, 2, 3, 9); "the full call" below is a case's D group.

The bars are the project's SGPR rule (tests/test_sgpr_gpu.py, head comment): per case the restatement
is evaluated by its two routes and their spread — a property of the references, never of the device
result — sets the bar:

    |F_dev − F_gpflow|  <=  max(10 · |F_gpflow − F_w|,     1e-12 · |F|)
    |g_dev − g_gpflow|  <=  max(10 · max|g_gpflow − g_w|,  1e-10 · (1 + max|g|))   per block (θ, noise, Z)
    predictions            max(10 · spread,                1e-10 · (1 + max|ref|))

and the bars themselves must be <= 1e-8·|F| and <= 1e-6·(1 + max|g|). Fitted losses (maxiter = 8)
track the existing solo path and the restatement's fit within max(1e3 · |fun_gpflow − fun_w|,
1e-9 · |fun|), the spread being that of the restatement fitted by its two routes here; the 1e3 allows
for a third summation order compounding over about nine evaluations (a judgement, not a measurement).
The two Periodic kernels are left out of the tracking on purpose: at maxiter = 8 the restatement's own
two routes end 4e-9 ... 7e-2 apart on them, because the line search branches on rounding; they are
covered by the "ragged" case and by the exact batch == alone check. Everything "bit for bit" is
compared with == / assert_array_equal. The measured errors are in profiles/sgpr_batch.md."""
import functools

import numpy as np
import pytest
import scipy.optimize

pytestmark = pytest.mark.gpu

import portfoliooptgp_amd as gpx  # noqa: E402
from portfoliooptgp_amd import _native as N  # noqa: E402
from portfoliooptgp_amd.engine import SGPRSmallEngine  # noqa: E402
from portfoliooptgp_amd.kernels import compile_spec  # noqa: E402
from portfoliooptgp_amd.trainer import ModelTrainer, mean_squared_error  # noqa: E402
from tests import sgpr_batch_cases as C  # noqa: E402
from tests import svgp_batch_cases as SC  # noqa: E402
from tests.sgpr_numpy import NumpySGPR  # noqa: E402
from tests.test_callers_gpu import PERIODIC, ref_kernels  # noqa: E402
from tests.test_gpu_parity import oracle_kernel  # noqa: E402

N_MAX, M_MAX = 4096, 32  # the path's limits: above or at every case's own size
REF_FAMILIES = ["se", "m12", "rq", "exp", "se+m12", "exp+per+lin", "exp+per", "se*m12"]  # ref_kernels(), in order


def _theta(gk, noise):
    row = np.ones(N.GPX_THETA_STRIDE)
    kp = gk.parameters
    for i, p in enumerate(kp):
        row[i] = p.value
    row[len(kp)] = noise
    return row


@functools.lru_cache(maxsize=None)
def case(name):
    X, Y, Z, gk, ok, s = C.build(name)
    return dict(X=X, Y=Y, Z=Z, gk=gk, ok=ok, noise=s, n=X.shape[0], M=Z.shape[0], D=X.shape[1])


def _blocks(g):
    return {"theta": np.asarray(g["theta"]), "noise": np.asarray([g["noise"]]), "Z": np.asarray(g["Z"])}


@functools.lru_cache(maxsize=None)
def reference(name):
    """The GPflow-route F and gradient blocks, the bars from the two routes' spread, cond(Kmm)."""
    c = case(name)
    om = NumpySGPR(c["ok"], c["X"], c["Y"], c["Z"], noise_variance=c["noise"])
    Fa, ga = om.elbo_and_grads("gpflow")
    Fb, gb = om.elbo_and_grads("w")
    ga, gb = _blocks(ga), _blocks(gb)
    tolF = max(10.0 * abs(Fa - Fb), 1e-12 * abs(Fa))
    tolg = {k: max(10.0 * float(np.abs(ga[k] - gb[k]).max()), 1e-10 * (1.0 + float(np.abs(ga[k]).max())))
            for k in ga}
    return dict(F=Fa, g=ga, tolF=tolF, tolg=tolg, cond=float(np.linalg.cond(om.kmm())))


def _groups():
    g = {}
    for name in C.NAMES:
        g.setdefault(C.CASES[name][2], []).append(name)
    return g


def _engine(names, nan_tails=False, n_max=N_MAX, m_max=M_MAX):
    """An engine holding the named cases in slots 0..; nan_tails: every slot's X / Y tail and the tail
    of its Z row are NaN."""
    D = case(names[0])["D"]
    eng = SGPRSmallEngine(len(names), n_max, m_max, D)
    for s, name in enumerate(names):
        c = case(name)
        spec = compile_spec(c["gk"], D)
        if nan_tails:
            eng.bind(s, np.full((n_max, D), np.nan), np.full(n_max, np.nan), spec, 1)
            eng.Z[s] = np.nan
        eng.bind(s, c["X"], c["Y"], spec, c["M"])
        eng.pack(s, _theta(c["gk"], c["noise"]), c["Z"])
    return eng


def _same(a, b):
    assert a[0] == b[0], (a[0], b[0])
    for x, y in zip(a[1:], b[1:]):
        np.testing.assert_array_equal(x, y)


@pytest.fixture(scope="module")
def full():
    """{case: outputs} from the full call of its D group (all slots active, in order)."""
    out = {}
    for D, names in _groups().items():
        eng = _engine(names)
        info = eng.elbo_grad(list(range(len(names))))
        assert not info.any(), info
        for s, name in enumerate(names):
            out[name] = eng.result(s)
    return out


def test_bound_and_gradients_vs_restatement(full):
    bad = []
    for name in C.NAMES:
        ref = reference(name)
        assert ref["cond"] <= C.COND_CAP, (name, ref["cond"])
        assert ref["tolF"] <= 1e-8 * abs(ref["F"]), (name, ref["tolF"], ref["F"])
        for k, t in ref["tolg"].items():
            assert t <= 1e-6 * (1.0 + float(np.abs(ref["g"][k]).max())), (name, k, t)
        F, gth, gZ = full[name]
        np_ = len(ref["g"]["theta"])
        got = {"theta": gth[:np_], "noise": gth[np_:np_ + 1], "Z": gZ}
        dF = abs(F - ref["F"])
        print(f"{name}: cond={ref['cond']:.3g} F={ref['F']:.17g} dF={dF:.3g} rel={dF / abs(ref['F']):.3g} "
              f"tolF={ref['tolF']:.3g}")
        assert np.all(gth[np_ + 1:] == 0.0), name
        if not dF <= ref["tolF"]:
            bad.append((name, "F", dF, ref["tolF"]))
        for k in got:
            err = float(np.abs(got[k] - ref["g"][k]).max())
            print(f"  {k}: err={err:.3g} rel={err / (1.0 + np.abs(ref['g'][k]).max()):.3g} tol={ref['tolg'][k]:.3g}")
            if not err <= ref["tolg"][k]:
                bad.append((name, k, err, ref["tolg"][k]))
    assert not bad, bad


def test_composition_invariance_bitwise(full):
    """A model's outputs from the full call == from the full call with the active list reversed == from a
    call of one slot of the shared object alone == from another object holding it alone (B = 1, its
    own N_max / M_max)."""
    for D, names in _groups().items():
        eng = _engine(names)
        eng.elbo_grad(list(range(len(names)))[::-1])
        for s, name in enumerate(names):
            _same(eng.result(s), full[name])
        eng.g_theta[:], eng.g_Z[:], eng.elbo[:] = 0.0, 0.0, 0.0
        eng.elbo_grad([len(names) - 1])  # one slot of the shared object alone
        _same(eng.result(len(names) - 1), full[names[-1]])
    for name in C.NAMES:
        c = case(name)
        solo = _engine([name], n_max=c["n"], m_max=c["M"])
        solo.elbo_grad([0])
        _same(solo.result(0), full[name])


def test_tails_are_not_read(full):
    for D, names in _groups().items():
        eng = _engine(names, nan_tails=True)
        info = eng.elbo_grad(list(range(len(names))))
        assert not info.any()
        for s, name in enumerate(names):
            _same(eng.result(s), full[name])


def test_predict_vs_restatement():
    rng = np.random.default_rng(8)
    bad = []
    for name, xs in (("ref", case("ref")["X"]), ("m32", rng.uniform(-1, 11, (333, 2)))):
        c = case(name)
        eng = _engine([name])
        om = NumpySGPR(c["ok"], c["X"], c["Y"], c["Z"], noise_variance=c["noise"])
        th = _theta(c["gk"], c["noise"])
        for add_noise, fn in ((False, om.predict_f), (True, om.predict_y)):
            (mo, vo), (mw, vw) = fn(xs, "gpflow"), fn(xs, "w")
            mu, var = eng.predict(0, th, c["Z"], xs, add_noise)
            assert mu.shape == (len(xs),) and var.shape == (len(xs),)
            for what, got, a, b in (("mean", mu, mo[:, 0], mw[:, 0]), ("var", var, vo[:, 0], vw[:, 0])):
                tol = max(10.0 * float(np.abs(a - b).max()), 1e-10 * (1.0 + float(np.abs(a).max())))
                err = float(np.abs(got - a).max())
                print(f"{name}: {'predict_y' if add_noise else 'predict_f'} {what} err={err:.3g} tol={tol:.3g}")
                if not err <= tol:
                    bad.append((name, add_noise, what, err, tol))
        mu0, var0 = eng.predict(0, th, c["Z"], np.zeros((0, c["D"])), False)
        assert mu0.shape == (0,) and var0.shape == (0,)
    assert not bad, bad


# ---- fits -----------------------------------------------------------------------------------------

OPTS = dict(maxiter=8)


def _days():
    return SC.days_xy(89, 3)


def _z0():
    return np.linspace(0, 88, 20)[:, None]


def _model(kernel, x, y, z=None):
    """GPflow's defaults: noise variance 1.0 trainable, Z trainable."""
    return gpx.models.SGPR((x, y), kernel, inducing_variable=_z0() if z is None else z)


def _same_result(a, b):
    np.testing.assert_array_equal(a.x, b.x)
    assert (a.fun, a.nit, a.nfev) == (b.fun, b.nit, b.nfev), ((a.fun, a.nit, a.nfev), (b.fun, b.nit, b.nfev))


def _solo(m):
    return gpx.optimizers.Scipy().minimize(m.training_loss, m.trainable_variables, options=OPTS)


def _restatement_fit(fam, x, y, route):
    om = NumpySGPR(oracle_kernel(fam), x, y, _z0(), noise_variance=1.0)

    def f(u):
        om.set_u(u)
        return om.loss_and_grad_u(route)

    return scipy.optimize.minimize(f, om.get_u(), jac=True, method="L-BFGS-B", options=OPTS)


def test_batch_fit_equals_solo_fit_and_tracks_existing_path_and_restatement():
    x, y = _days()
    opt = gpx.optimizers.Scipy()
    batch = opt.minimize_sgpr_batch([_model(k, x, y) for k in ref_kernels()], options=OPTS)
    for i, k in enumerate(ref_kernels()):
        alone = opt.minimize_sgpr_batch([_model(k, x, y)], options=OPTS)[0]
        _same_result(batch[i], alone)
    bad = []
    for i, k in enumerate(ref_kernels()):
        if i in PERIODIC:
            continue
        ref = _solo(_model(k, x, y))
        ra, rb = (_restatement_fit(REF_FAMILIES[i], x, y, r) for r in ("gpflow", "w"))
        tol = max(1e3 * abs(ra.fun - rb.fun), 1e-9 * abs(ra.fun))
        d_solo, d_rest = abs(batch[i].fun - ref.fun), abs(batch[i].fun - ra.fun)
        print(f"{REF_FAMILIES[i]}: fun={batch[i].fun:.15g} nfev={batch[i].nfev} |batch-solo|={d_solo:.3g} "
              f"|batch-restatement|={d_rest:.3g} |solo-restatement|={abs(ref.fun - ra.fun):.3g} "
              f"routes' spread={abs(ra.fun - rb.fun):.3g} tol={tol:.3g}")
        if not d_solo <= tol:
            bad.append((REF_FAMILIES[i], "solo", d_solo, tol))
        if not d_rest <= tol:
            bad.append((REF_FAMILIES[i], "restatement", d_rest, tol))
    assert not bad, bad


def test_per_model_data_and_written_back_state():
    """Each model its own (X, Y) of a different n, and the fitted values are in the models."""
    x, y = _days()
    K = gpx.kernels
    kinds, ns = (K.SquaredExponential, K.Matern12, K.RationalQuadratic), (89, 40, 11)
    z = np.linspace(0, 88, 10)[:, None]
    ms = [_model(k(), x[:n], y[:n], z.copy()) for k, n in zip(kinds, ns)]
    res = gpx.optimizers.Scipy().minimize_sgpr_batch(ms, options=OPTS)
    for m, r, k, n in zip(ms, res, kinds, ns):
        alone = _model(k(), x[:n], y[:n], z.copy())
        ra = gpx.optimizers.Scipy().minimize_sgpr_batch([alone], options=OPTS)[0]
        _same_result(r, ra)
        assert r.nit >= 1 and not np.array_equal(m.inducing_variable.Z.value, z)
        np.testing.assert_array_equal(m.inducing_variable.Z.value, alone.inducing_variable.Z.value)
        np.testing.assert_array_equal(m.theta_row(), alone.theta_row())
        np.testing.assert_array_equal(
            np.concatenate([np.atleast_1d(v.numpy()).ravel() for v in m.trainable_variables]), r.x)


def test_over_limit_model_takes_the_existing_path():
    x, y = _days()
    K = gpx.kernels
    opt = gpx.optimizers.Scipy()
    mk = lambda: [_model(K.SquaredExponential(), x, y),  # noqa: E731
                  _model(K.Matern12(), x, y, np.linspace(0, 88, 40)[:, None]),
                  _model(K.Matern32(), x, y, np.linspace(0, 88, 7)[:, None])]
    ms = mk()
    res = opt.minimize_sgpr_batch(ms, options=OPTS)
    ref = mk()
    _same_result(res[1], _solo(ref[1]))
    for i in (0, 2):
        _same_result(res[i], opt.minimize_sgpr_batch([ref[i]], options=OPTS)[0])
    # prediction: the bound slots, and the over-limit model by its own engine
    preds = gpx.models.predict_f_sgpr_batch(ms, [x, x, x])
    m1, v1 = ref[1].predict_f(x)
    np.testing.assert_array_equal(preds[1][0].numpy(), m1.numpy())
    np.testing.assert_array_equal(preds[1][1].numpy(), v1.numpy())
    for (mu, var), m in zip(preds, ms):
        assert tuple(mu.shape) == (89, 1) and tuple(var.shape) == (89, 1)
    for i in (0, 2):  # the fused predict agrees with the model's own engine at the fitted state
        mo, vo = ms[i].predict_f(x)
        np.testing.assert_allclose(preds[i][0].numpy(), mo.numpy(), rtol=1e-7, atol=1e-9)
        np.testing.assert_allclose(preds[i][1].numpy(), vo.numpy(), rtol=1e-7, atol=1e-9)
    py = gpx.models.predict_f_sgpr_batch(ms[:1], [x], add_noise=True)[0]
    np.testing.assert_array_equal(py[0].numpy(), preds[0][0].numpy())
    np.testing.assert_allclose(py[1].numpy() - preds[0][1].numpy(), ms[0].likelihood.variance.value, rtol=1e-9)
    for m in (ms[0], ms[1]):
        mu0, var0 = gpx.models.predict_f_sgpr_batch([m], [np.zeros((0, 1))])[0]
        assert tuple(mu0.shape) == (0, 1) and tuple(var0.shape) == (0, 1)


def _not_pd_models(x, y):
    K = gpx.kernels
    z = _z0()
    z[1] = z[0]  # two identical inducing rows under a variance of 2^40: the second pivot of Kmm is exactly 0
    bad = _model(K.SquaredExponential(variance=2.0 ** 40), x, y, z)
    return [_model(K.Matern32(), x, y), bad, _model(K.Exponential(), x, y)]


def test_not_pd_raises_by_default_and_inf_keeps_the_others():
    x, y = _days()
    opt = gpx.optimizers.Scipy()
    with pytest.raises(gpx.NotPositiveDefiniteError):
        _solo(_not_pd_models(x, y)[1])
    with pytest.raises(gpx.NotPositiveDefiniteError) as e:
        opt.minimize_sgpr_batch(_not_pd_models(x, y), options=OPTS)
    assert e.value.info == 2
    ms = _not_pd_models(x, y)
    res = opt.minimize_sgpr_batch(ms, options=OPTS, on_not_pd="inf")
    assert len(res) == 3 and res[1].fun == float("inf")
    ref = _not_pd_models(x, y)
    for i in (0, 2):
        _same_result(res[i], opt.minimize_sgpr_batch([ref[i]], options=OPTS)[0])


def test_train_sgpr_model_matches_the_loop_of_solo_fits():
    x, y = _days()
    ks = [k for i, k in enumerate(ref_kernels()) if i not in PERIODIC]
    solo_mse = []
    for k in [k for i, k in enumerate(ref_kernels()) if i not in PERIODIC]:
        m = _model(k, x, y)
        _solo(m)
        solo_mse.append(mean_squared_error(y, m.predict_f(x)[0].numpy()))
    s = sorted(solo_mse)
    print("solo MSE", solo_mse)
    assert (s[1] - s[0]) / s[0] > 1e-3, solo_mse  # the winner is not decided by a tie
    tr = ModelTrainer(ks)
    best_kernel, best_mse, best_model = tr.train_sgpr_model(x, y, n_inducing=20, maxiter=8)
    for m in tr.last_models:
        np.testing.assert_array_equal(np.asarray(m.data[0]), x)
    mses = [mean_squared_error(y, p[0].numpy())
            for p in gpx.models.predict_f_sgpr_batch(tr.last_models, [x] * len(ks))]
    print("batch MSE", mses)
    for a, b in zip(mses, solo_mse):
        assert a == pytest.approx(b, rel=1e-5)
    assert best_kernel is ks[int(np.argmin(solo_mse))]
    assert best_mse == min(mses) and best_model is tr.last_models[int(np.argmin(solo_mse))]
