"""GPR mean functions on the device: every evaluation route against the numpy reference of
tests/test_mean_functions.py (the oracle's GPR on the residual y − m(X; β), plus Φᵀα), the
predictions, the bitwise rules, fits and the refusals.

Each route case holds five slots on the same series — Constant, Linear, Polynomial(2), a zero-mean
slot and Constant(0.0) — evaluated in one mixed call; the route the case is meant to take is asserted
through last_timing() / band_class. x are raw day offsets, β is away from zero. The noise variance is
0.05 so that cond(K + σn²I) stays near 10²–10³ on every route: the bars below are the project's
(check_loss 1e-9, check_grad 1e-6) without any κ allowance.

Bars: logML and the kernel / noise gradient block as tests/test_gpu_parity.py; mean-gradient
component k within 1e-6 · Σ_j |α_j ∂m(x_j)/∂β_k| (the dot product's own scale, so the largest of the
components — they differ by five orders of magnitude — cannot hide the smallest).
"""

import numpy as np
import pytest
import scipy.optimize

pytestmark = pytest.mark.gpu

import portfoliooptgp_amd as gpx  # noqa: E402
from portfoliooptgp_amd import _native as N  # noqa: E402
from portfoliooptgp_amd.engine import Engine  # noqa: E402
from portfoliooptgp_amd.kernels import compile_spec  # noqa: E402
from portfoliooptgp_amd.models import predict_f_batch  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402
from tests.test_band_gpu import _Env, _engine, _theta  # noqa: E402
from tests.test_gpu_parity import check_grad, check_loss, check_mean, check_var  # noqa: E402
from tests.test_mean_functions import mean_basis, ref_eval, series  # noqa: E402

K = gpx.kernels
MF = gpx.mean_functions
NOISE = 0.05
KINDS = [("constant", N.GPX_MEAN_CONSTANT, 0), ("linear", N.GPX_MEAN_LINEAR, 0), ("polynomial", N.GPX_MEAN_POLYNOMIAL, 2)]


def betas(n):
    """β of the three kinds for a series of n raw day offsets (near its trend, not at it)."""
    return {"constant": np.array([0.7]), "linear": np.array([-1.4 / n, 0.9]),
            "polynomial": np.array([0.7, -1.4 / n, 1.9 / (n * n)])}


def spec_of(kind, deg, ncoef):
    return N.GpxMeanSpec(kind, deg, ncoef, 0)


# a route's kernel: (gpx kernel factory, oracle kernel factory at θ, kernel θ in GPflow order)
def _se(ell, var=0.8):
    return (lambda: K.SquaredExponential(), lambda: O.OSquaredExponential(variance=var, lengthscales=ell), (ell, var))


def _m12(ell, var=0.8):
    return (lambda: K.Matern12(), lambda: O.OMatern12(variance=var, lengthscales=ell), (ell, var))


# route -> N, kernel, engine band route (default sweeps), a per-call library switch, and the check of
# the mixed call's timing counters t and band classes c that names the route taken
ROUTES = {
    # the fused small-problem launches and the dense chain (no band tables below 8 blocks)
    "small64": dict(n=50, k=_se(6.0), check=lambda t, c: t.band_evals == 0),
    "small128": dict(n=100, k=_se(6.0), check=lambda t, c: t.band_evals == 0),
    "dense251": dict(n=251, k=_se(6.0), check=lambda t, c: t.band_evals == 0),
    # N = 512: the band16 sweeps at Q = 1 and Q = 3, the reduction route, the 64-row fused sweeps
    "band16_q1": dict(n=512, k=_se(0.3), check=lambda t, c: t.band16_evals == 5 and set(c) == {1}),
    "band16_q3": dict(n=512, k=_se(1.0), check=lambda t, c: t.band16_evals == 5 and set(c) == {3}),
    "bcr_q3": dict(n=512, k=_se(1.0), route="bcr", check=lambda t, c: t.bcr_evals == 5 and t.band16_evals == 0),
    "fused64_p1": dict(n=512, k=_m12(0.02), env=("GPX_BAND16", "0"),
                       check=lambda t, c: t.band_fused_launches >= 1 and t.band16_evals == 0 and t.band_evals == 5),
    # N = 1024: the per-block band at p = 3, and SE problems of band16 width Q = 6 (reachable at this
    # size): the wide one-wavefront sweeps on the sweeps route, the block-128 reduction on the BCR route
    "band_p3": dict(n=1024, k=_se(4.5), check=lambda t, c: t.band_evals == 5 and t.band16_evals == 0
                    and t.band_fused_launches == 0 and set(c) <= {19, 35}),
    "band16_q6": dict(n=1024, k=_se(2.3), check=lambda t, c: t.band16_evals == 5 and t.bcr_wide_evals == 0
                      and set(c) == {6}),
    "bcr_wide_q6": dict(n=1024, k=_se(2.3), route="bcr",
                        check=lambda t, c: t.bcr_wide_evals == 5 and t.band16_evals == 0 and set(c) == {6}),
}


class RouteCase:
    """The five-slot engine of one route, its mixed-call results and the references, built once."""

    def __init__(self, name):
        r = ROUTES[name]
        self.name, self.n = name, r["n"]
        mk, mo, th = r["k"]
        self.x, self.y = series(self.n)
        self.ok = mo()
        self.ktheta = th
        self.env = _Env(*r["env"]) if "env" in r else None
        self.kern = mk()
        self.np_ = len(th)
        self.beta = betas(self.n)
        prev = gpx.set_default_band_route(r.get("route", "sweeps"))
        try:
            self.eng = _engine([self.x] * 5, [self.y] * 5, self.kern)
            self.eng0 = _engine([self.x], [self.y], mk())  # the same model with no mean anywhere in its batch
        finally:
            gpx.set_default_band_route(prev)
        for b, (kn, kind, deg) in enumerate(KINDS):
            self.eng.set_mean(b, spec_of(kind, deg, len(self.beta[kn])))
        self.eng.set_mean(4, spec_of(N.GPX_MEAN_CONSTANT, 0, 1))
        rows = [th + (NOISE,) + tuple(self.beta[kn]) for kn, _, _ in KINDS] + [th + (NOISE,), th + (NOISE, 0.0)]
        self.theta = _theta(self.eng, rows)
        self.theta0 = _theta(self.eng0, [th + (NOISE,)])
        self.check = r["check"]
        self.refs = [ref_eval(self.x, self.y, self.ok, NOISE, kn, self.beta[kn], deg) for kn, _, deg in KINDS]
        # ∂θ/∂u of the kernel parameters and the noise, to bring the oracle's ∂/∂u back to ∂/∂θ
        om = O.OGPR(self.x, self.y, self.ok, noise_variance=NOISE)
        self.dth = np.array([p.dtheta_du() for p in self.ok.params()] + [om.noise.dtheta_du()])

    def __enter__(self):
        if self.env:
            self.env.__enter__()
        return self

    def __exit__(self, *a):
        if self.env:
            self.env.__exit__(*a)


_CASES = {}


def case(name):
    c = _CASES.get(name)
    if c is None:
        c = _CASES[name] = RouteCase(name)
    return c


@pytest.mark.parametrize("name", list(ROUTES))
def test_route_against_reference_and_bitwise(name):
    with case(name) as c:
        eng, th, P = c.eng, c.theta, c.np_ + 1
        act = [0, 1, 2, 3, 4]
        cls = [int(v) for v in eng.band_class(act, th)]
        eng.reset_timing()
        lml, grad, info = eng.lml_grad(act, th)
        t = eng.last_timing()
        assert not info.any(), info
        assert c.check(t, cls), (name, cls, t.band_evals, t.band16_evals, t.bcr_evals, t.bcr_wide_evals,
                                 t.band_fused_launches)
        assert t.band_fallbacks == 0
        for b, (kn, _, _) in enumerate(KINDS):
            l_ref, gu_ref, gm_ref, alpha, Phi = c.refs[b]
            print(f"{name}/{kn}: logML {lml[b]:.12e} ref {l_ref:.12e}; mean grad {grad[b, P:P + Phi.shape[1]]} ref {gm_ref}")
            check_loss(lml[b], l_ref)
            check_grad(grad[b, :P], -gu_ref / c.dth)
            scale = np.abs(alpha[:, None] * Phi).sum(0)
            err = np.abs(grad[b, P:P + Phi.shape[1]] - gm_ref)
            assert np.all(err <= 1e-6 * scale), (name, kn, err, scale)
        # Constant(0.0) and the zero-mean slot of the mixed call: the bits of the model without a mean
        eng0 = c.eng0
        eng0.reset_timing()
        l0, g0, i0 = eng0.lml_grad([0], c.theta0)
        assert not i0.any()
        for b in (3, 4):
            assert lml[b] == l0[0] and np.array_equal(grad[b, :P], g0[0, :P]), (name, b, lml[b], l0[0])
        _, _, gm0, alpha0, _ = ref_eval(c.x, c.y, c.ok, NOISE, "constant", [0.0])
        assert abs(grad[4, P] - gm0[0]) <= 1e-6 * np.abs(alpha0).sum()  # (Σ_j α_j of the zero-mean model)
        # a problem alone in its call: the bits it has in the mixed call
        for b, nc in zip(act, (1, 2, 3, 0, 1)):
            l1, g1, i1 = eng.lml_grad([b], th)
            assert not i1.any()
            assert l1[b] == lml[b] and np.array_equal(g1[b, :P + nc], grad[b, :P + nc]), (name, b)


@pytest.mark.parametrize("name", list(ROUTES))
def test_route_predictions(name):
    with case(name) as c:
        eng, th, n = c.eng, c.theta, c.n
        rng = np.random.default_rng(11)
        xs = np.sort(rng.uniform(0.0, n + 3.0, 9))[:, None]
        act = [0, 1, 2, 3]
        var_k = c.ktheta[1]
        oms, m_new, m_trn = [], [], []
        for b, (kn, _, deg) in enumerate(KINDS):
            Phi = mean_basis(kn, c.x, deg)
            oms.append(O.OGPR(c.x, c.y.reshape(-1) - Phi @ c.beta[kn], c.ok, noise_variance=NOISE))
            m_new.append(mean_basis(kn, xs, deg) @ c.beta[kn])
            m_trn.append(Phi @ c.beta[kn])
        oms.append(O.OGPR(c.x, c.y, c.ok, noise_variance=NOISE))
        m_new.append(np.zeros(len(xs)))
        m_trn.append(np.zeros(n))
        yscale = float(np.abs(c.y).max())
        mf, vf, _ = eng.predict(act, th, [xs] * 4, False)
        my, vy, _ = eng.predict(act, th, [xs] * 4, True)
        mc, cc, _ = eng.predict(act, th, [xs] * 4, False, full_cov=True)
        # the train-input path, from the factor the route's own evaluation leaves behind
        _, _, inf = eng.lml_grad(act, th)
        assert not inf.any()
        mt, vt, _ = eng.predict(act, th, [c.x] * 4, False)
        for b in act:
            mo, vo = oms[b].predict_f(xs)
            _, co = oms[b].predict_f(xs, full_cov=True)
            ref = mo[:, 0] + m_new[b]
            check_mean(mf[b].cpu().numpy(), ref, yscale=yscale)
            check_mean(my[b].cpu().numpy(), ref, yscale=yscale)
            check_mean(mc[b].cpu().numpy(), ref, yscale=yscale)
            # the variances are the zero-mean model's on the residual data
            check_var(vf[b].cpu().numpy(), vo, var_k)
            check_var(vy[b].cpu().numpy(), vo + NOISE, var_k)
            assert np.abs(cc[b].cpu().numpy() - co).max() <= 1e-5 * np.abs(co).max() + 1e-10 * var_k
            mto, vto = oms[b].predict_f(c.x)
            check_mean(mt[b].cpu().numpy(), mto[:, 0] + m_trn[b], yscale=yscale)
            check_var(vt[b].cpu().numpy(), vto, var_k)
        # the variances do not depend on β at all: the zero-mean slot's, to rounding
        for b in (0, 1, 2):
            np.testing.assert_allclose(vf[b].cpu().numpy(), vf[3].cpu().numpy(), rtol=1e-9, atol=1e-12 * var_k)


@pytest.mark.parametrize("name", ["small64", "dense251", "band16_q3"])
def test_predict_after_a_beta_only_change(name):
    """The factor cache: predict, change only β, predict again. α depends on β, so the second
    prediction must be the reference's at the new β (a stale α would give the old one plus the
    difference in m(X*) only); far outside the data, where k(X*, X) is exactly zero, the mean moves
    by exactly the difference in m(X*)."""
    with case(name) as c:
        eng, n = c.eng, c.n
        th1 = c.theta.copy()
        th2 = c.theta.copy()
        P = c.np_ + 1
        b, (kn, _, deg) = 2, KINDS[2]
        beta2 = c.beta[kn] * np.array([0.5, 1.5, 0.75])
        th2[b, P:P + 3] = beta2
        far = 1e4  # (SE: k = 0 exactly in fp64 beyond ~39 ℓ, and ℓ <= 6 here)
        xs = np.array([3.3, n / 2 + 0.4, n - 1.7, far, far + 7.0])[:, None]
        eng.lml_grad([b], th1)  # the factor at β1 is cached
        m1, v1, _ = eng.predict([b], th1, [xs], False)
        m2, v2, _ = eng.predict([b], th2, [xs], False)
        mt2, _, _ = eng.predict([b], th2, [c.x], False)
        Phi, Phis = mean_basis(kn, c.x, deg), mean_basis(kn, xs, deg)
        om2 = O.OGPR(c.x, c.y.reshape(-1) - Phi @ beta2, c.ok, noise_variance=NOISE)
        yscale = float(np.abs(c.y).max())
        check_mean(m2[0].cpu().numpy(), om2.predict_f(xs)[0][:, 0] + Phis @ beta2, yscale=yscale)
        check_mean(mt2[0].cpu().numpy(), om2.predict_f(c.x)[0][:, 0] + Phi @ beta2, yscale=yscale)
        assert np.abs(m2[0].cpu().numpy()[:3] - m1[0].cpu().numpy()[:3]).max() > 1e-3  # (it moved)
        np.testing.assert_array_equal(v1[0].cpu().numpy(), v2[0].cpu().numpy())
        d = (m2[0].cpu().numpy() - m1[0].cpu().numpy())[3:]
        dm = (Phis @ beta2 - Phis @ c.beta[kn])[3:]
        rounding = 16 * np.finfo(float).eps * (np.abs(Phis[3:] * beta2).sum(1) + np.abs(Phis[3:] * c.beta[kn]).sum(1))
        assert np.all(np.abs(d - dm) <= rounding), (d, dm)
        # and back: the cached factor at β2 must not serve β1
        m1b, _, _ = eng.predict([b], th1, [xs], False)
        np.testing.assert_array_equal(m1b[0].cpu().numpy(), m1[0].cpu().numpy())


def test_model_surface_solo():
    """models.GPR with each mean kind through the pooled solo engine, one after another on the same
    slot (the pool rebinds it, which resets the mean), against the reference."""
    n = 100
    x, y = series(n)
    ok = O.OSquaredExponential(variance=0.8, lengthscales=6.0)
    bt = betas(n)
    models = []
    for kn, mf in [("constant", MF.Constant(bt["constant"])), ("linear", MF.Linear(A=bt["linear"][:1, None], b=bt["linear"][1:])),
                   ("polynomial", MF.Polynomial(2, w=bt["polynomial"][:, None])), (None, None), (None, MF.Zero())]:
        m = gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential(lengthscales=6.0, variance=0.8),
                           mean_function=mf, noise_variance=NOISE)
        models.append((kn, m))
    xs = np.linspace(-2.0, n + 2.0, 6)[:, None]
    for rep in range(2):  # (twice: every model follows another kind on the pooled slot)
        for kn, m in models:
            loss, g = m.loss_and_grad_unconstrained()
            if kn is None:
                om = O.OGPR(x, y, ok, noise_variance=NOISE)
                lo, go = om.loss_and_grad_u()
                check_loss(loss, lo)
                check_grad(g, go)
                mo = om.predict_f(xs)[0][:, 0]
            else:
                deg = 2 if kn == "polynomial" else 0
                l_ref, gu_ref, gm_ref, alpha, Phi = ref_eval(x, y, ok, NOISE, kn, bt[kn], deg)
                check_loss(loss, -l_ref)
                check_grad(g[:3], gu_ref)
                assert np.all(np.abs(g[3:] + gm_ref) <= 1e-6 * np.abs(alpha[:, None] * Phi).sum(0))
                om = O.OGPR(x, y.reshape(-1) - Phi @ bt[kn], ok, noise_variance=NOISE)
                mo = om.predict_f(xs)[0][:, 0] + mean_basis(kn, xs, deg) @ bt[kn]
            mean, var = m.predict_f(xs)
            check_mean(mean.numpy(), mo, yscale=float(np.abs(y).max()))
            check_var(var.numpy(), om.predict_f(xs)[1], 0.8)


def _fit_models(x, y, n):
    """Four models for one batch: the Polynomial(2) fit of the solo test and three others."""
    w0 = np.polyfit(x[:, 0], y.reshape(-1), 2)[::-1]
    w0 = np.array([float(f"{v:.2e}") for v in w0])  # (a start near the trend, two digits)

    def base(mf):
        m = gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential(lengthscales=5.0, variance=0.5),
                           mean_function=mf, noise_variance=NOISE)
        gpx.set_trainable(m.likelihood.variance, False)
        return m
    return w0, [base(MF.Polynomial(2, w=w0[:, None])), base(MF.Constant([0.1])), base(None),
                base(MF.Linear(A=[[w0[1]]], b=[w0[0]]))]


def test_fits_solo_against_scipy_and_batch_bitwise():
    """Solo Scipy().minimize on N = 251 with Polynomial(2) and fixed noise reaches the loss of
    scipy.optimize.minimize on the reference function from the same start (1e-4 relative, the θ*
    tolerance of tests/test_c2_parity_gpu.py); the same model inside minimize_batch of four gives
    the solo result bit for bit."""
    n = 251
    x, y = series(n)
    w0, ms = _fit_models(x, y, n)
    solo = ms[0]
    x0 = np.array([p.unconstrained for p in solo.kernel.parameters] + list(w0))
    ok = O.OSquaredExponential(variance=0.5, lengthscales=5.0)
    kp = ok.params()

    def ref_fun(u):
        for p, v in zip(kp, u[:2]):
            p.set_u(float(v))
        lml, gu, gm, _, _ = ref_eval(x, y, ok, NOISE, "polynomial", u[2:], 2, noise_trainable=False)
        return -lml, np.concatenate([gu, -gm])

    ref = scipy.optimize.minimize(ref_fun, x0, jac=True, method="L-BFGS-B", options=dict(maxiter=100))
    res = gpx.optimizers.Scipy().minimize(solo.training_loss, solo.trainable_variables, options=dict(maxiter=100))
    print(f"solo fit: loss* {res.fun:.10f} (nfev {res.nfev}), scipy on the reference {ref.fun:.10f} (nfev {ref.nfev})")
    assert abs(res.fun - ref.fun) <= 1e-4 * abs(ref.fun), (res.fun, ref.fun)
    _, ms2 = _fit_models(x, y, n)
    out = gpx.optimizers.Scipy().minimize_batch(ms2, options=dict(maxiter=100))
    assert out[0].fun == res.fun and np.array_equal(out[0].x, res.x) and out[0].nfev == res.nfev
    assert np.array_equal(ms2[0].mean_function.w.value, solo.mean_function.w.value)
    # the batch's models predict together, each with its own mean
    xs = np.linspace(0.0, n + 4.0, 5)[:, None]
    both = predict_f_batch(ms2, [xs] * 4)
    m_solo, v_solo = solo.predict_f(xs)
    np.testing.assert_allclose(both[0][0].numpy(), m_solo.numpy(), rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(both[0][1].numpy(), v_solo.numpy(), rtol=1e-12, atol=1e-15)


def test_refusals_leave_the_batch_usable():
    n = 512
    x, y = series(n)
    spec = compile_spec(K.SquaredExponential(), 1)
    th = np.ones((1, N.GPX_THETA_STRIDE))
    th[0, :3] = (1.0, 0.8, NOISE)
    poly = spec_of(N.GPX_MEAN_POLYNOMIAL, 2, 3)
    # band storage
    eb = Engine([x], [y], [spec], band_storage=True)
    with pytest.raises(N.GPXError, match="band-storage"):
        eb.set_mean(0, poly)
    assert not eb.has_mean
    l_b, _, i_b = eb.lml_grad([0], th)
    # deferral, both orders
    ed = Engine([x], [y], [spec])
    l_d, _, i_d = ed.lml_grad([0], th)
    assert not i_b.any() and not i_d.any() and abs(l_b[0] - l_d[0]) <= 1e-9 * abs(l_d[0])
    ed.set_deferred(1)
    with pytest.raises(N.GPXError, match="deferred"):
        ed.set_mean(0, poly)
    ed.set_deferred(-1)
    ed.set_mean(0, poly)
    with pytest.raises(N.GPXError, match="mean function"):
        ed.set_deferred(1)
    th2 = th.copy()
    th2[0, 3:6] = betas(n)["polynomial"]
    l2, g2, i2 = ed.lml_grad([0], th2)
    l_ref = ref_eval(x, y, O.OSquaredExponential(variance=0.8, lengthscales=1.0), NOISE, "polynomial", th2[0, 3:6], 2)[0]
    assert not i2.any()
    check_loss(l2[0], l_ref)
    # bad specs and an over-full row
    for bad in (spec_of(7, 0, 1), spec_of(N.GPX_MEAN_POLYNOMIAL, 5, 6), spec_of(N.GPX_MEAN_LINEAR, 0, 3)):
        with pytest.raises(N.GPXError):
            ed.set_mean(0, bad)
    th2[0, 4] = np.nan
    with pytest.raises(N.GPXError, match="finite"):
        ed.lml_grad([0], th2)
    th2[0, 4] = -0.25  # (negative and zero coefficients are fine)
    assert not ed.lml_grad([0], th2)[2].any()
    # a rebind leaves the slot zero-mean: the bits of a batch that never had a mean
    ed.rebind(0, x, y, spec)
    assert not ed.has_mean
    l3, _, _ = ed.lml_grad([0], th)
    assert l3[0] == l_d[0]
    # minimize_stream refuses a model with a mean before any device call
    ms = [gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential(), mean_function=MF.Polynomial(2))]
    with pytest.raises(NotImplementedError, match="minimize_stream"):
        gpx.optimizers.Scipy().minimize_stream(ms, width=1)
