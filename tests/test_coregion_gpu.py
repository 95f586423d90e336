"""GPR with a Coregion kernel on the GPU against the CPU reference of tests/coregion_numpy.py: values
from the oracle's GPR with the Coregion factor restated in numpy, gradients from the torch-fp64
autograd restatement (validated against central differences on the CPU, tests/test_coregion_api.py).

Sizes: N = 5 and 60 (Np = 64), 67 (Np = 128: both on the launch chain, the Coregion route of the
small sizes), 200 (Np = 256: the recursion and off-diagonal 64-tiles in the contraction), 600
(Np = 640: the 128-tile instances). Bars of tests/test_gpu_parity.py:
  logML     (1e-9 + 1e-14 κ)·max(1, |ref|)          gradient  1e-6·max|g_ref|
  mean      1e-6·max|ref| + 1e-14 κ·max(1, max|y|)  variance  1e-5·|ref| + 1e-10·σ²_max
"""
import ctypes
import functools

import numpy as np
import pytest
import scipy.optimize

pytestmark = pytest.mark.gpu

import portfoliooptgp_amd as gpx  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402
from portfoliooptgp_amd import _native as N  # noqa: E402
from portfoliooptgp_amd import trainer  # noqa: E402
from portfoliooptgp_amd.engine import Engine  # noqa: E402
from portfoliooptgp_amd.kernels import compile_spec  # noqa: E402
from tests import coregion_numpy as C  # noqa: E402
from tests.test_gpu_parity import check_grad, check_loss, check_mean, check_var  # noqa: E402

K = gpx.kernels


@functools.lru_cache(maxsize=None)
def _reference(i):
    """(oracle values at N* in {1, N + 1}, restatement gradient with trainable / frozen noise, the
    prediction inputs) of PARITY_CASES[i]: computed once, shared, never modified."""
    c = C.PARITY_CASES[i]
    rng = np.random.default_rng(2000 + i)
    xnews = (C.prediction_inputs(c, 1, rng), C.prediction_inputs(c, c["n"] + 1, rng))
    ref = C.oracle_values(c, xnews)
    g = C.TorchCoregion(c).loss_and_grad()[1]
    g_fixed = C.TorchCoregion(c, trainable_noise=False).loss_and_grad()[1]
    return ref, g, g_fixed, xnews


@pytest.mark.parametrize("i", range(len(C.PARITY_CASES)), ids=[C.case_id(c) for c in C.PARITY_CASES])
def test_parity_at_fixed_theta(i):
    c = C.PARITY_CASES[i]
    ref, g_ref, g_fixed_ref, xnews = _reference(i)
    cond = ref["cond"]
    m = C.gpx_model(c)
    assert any(m._spec.terms[t].kind == N.GPX_COREGION for t in range(m._spec.n_terms))
    loss, g = m.loss_and_grad_unconstrained()
    check_loss(loss, ref["loss"], cond)
    check_grad(g, g_ref)
    if c["layout"] == "empty":
        # an asset without rows: exactly zero ∂loss/∂(its W row, its κ) — reference and device
        slots = C.TorchCoregion(c).coregion_slots(c["P"] - 1)
        assert np.all(g_ref[slots] == 0.0) and np.all(g[slots] == 0.0), (g_ref[slots], g[slots])
    gpx.set_trainable(m.likelihood.variance, False)
    _, g2 = m.loss_and_grad_unconstrained()
    check_grad(g2, g_fixed_ref)
    yscale = float(np.abs(m.data[1].numpy()).max())
    for xn, (fm, fv, fc) in zip(xnews, ref["pred"]):
        s2 = max(float(np.max(fv)), 1.0)
        mu, var = m.predict_f(xn)
        check_mean(mu.numpy(), fm, cond, yscale)
        check_var(var.numpy(), fv, s2)
        _, vy = m.predict_y(xn)
        check_var(vy.numpy(), fv + c["noise"], s2)
        mu2, cov = m.predict_f(xn, full_cov=True)
        check_mean(mu2.numpy(), fm, cond, yscale)
        assert cov.shape == (1, len(xn), len(xn))
        check_var(cov.numpy()[0], fc, s2)  # (elementwise: |Δ| <= 1e-5 |ref| + 1e-10 σ²_max)


# ---------------------------------------------------------------------------- identities
def _set_coregion(k, W, kappa):
    cg = [t for t in k._terms() if isinstance(t, K.Coregion)][0]
    cg.W.assign(W)
    cg.kappa.assign(kappa)
    return k


def test_independent_outputs_equal_the_single_asset_models():
    """W = 0, κ = 1: B = I, so the stacked model is P independent GPRs sharing the partner's θ and
    σn². Its loss is the sum of the P single-asset losses from the existing isotropic path, its
    gradient in (ℓ, σ², σn²) the sum of theirs. N_total = 200, P = 3."""
    P, ell, var, noise = 3, 1.3, 1.7, 1e-2
    c = C.case([("se", 0, 1, ell, var, None)], P, 1, 200, 1, noise=noise, seed=40, layout="perm")
    X, Y = C.make_data(c)
    k = _set_coregion(K.SquaredExponential(lengthscales=ell, variance=var, active_dims=[0])
                      * K.Coregion(P, 1, active_dims=[1]), np.zeros((P, 1)), np.ones(P))
    m = gpx.models.GPR((X, Y), kernel=k, noise_variance=noise)
    loss, g = m.loss_and_grad_unconstrained()
    loss_sum, g_sum, cond = 0.0, np.zeros(3), 1.0
    for p in range(P):
        sel = X[:, 1] == p
        mp = gpx.models.GPR((X[sel, :1], Y[sel]), kernel=K.SquaredExponential(lengthscales=ell, variance=var),
                            noise_variance=noise)
        lp, gp = mp.loss_and_grad_unconstrained()
        loss_sum += lp
        g_sum += gp
        om = O.OGPR(X[sel, :1], Y[sel], O.OSquaredExponential(variance=var, lengthscales=ell), noise_variance=noise)
        cond = max(cond, float(np.linalg.cond(om._Ky())))
    check_loss(loss, loss_sum, cond)
    check_grad(g[[0, 1, -1]], g_sum)


@pytest.mark.parametrize("n", [67, 200])
def test_one_output_equals_a_rescaled_variance(n):
    """P = 1: SE(σ²) × Coregion(1, 1) with W = [[w]], κ = [k] is SE(variance = σ²(w² + k))."""
    w, kap, var, ell, noise = -0.8, 0.45, 1.6, 1.2, 1e-2
    rng = np.random.default_rng(60 + n)
    F = rng.standard_normal((n, 2))
    Y = (np.sin(F[:, 0]) + 0.1 * rng.standard_normal(n))[:, None]
    X = np.concatenate([F, np.zeros((n, 1))], axis=1)
    k = _set_coregion(K.SquaredExponential(lengthscales=ell, variance=var, active_dims=[0, 1])
                      * K.Coregion(1, 1, active_dims=[2]), [[w]], [kap])
    m = gpx.models.GPR((X, Y), kernel=k, noise_variance=noise)
    v1 = var * (w * w + kap)
    m1 = gpx.models.GPR((F, Y), kernel=K.SquaredExponential(lengthscales=ell, variance=v1), noise_variance=noise)
    cond = float(np.linalg.cond(O.OGPR(F, Y, O.OSquaredExponential(variance=v1, lengthscales=ell),
                                       noise_variance=noise)._Ky()))
    check_loss(float(m.training_loss()), float(m1.training_loss()), cond)
    Fn = rng.standard_normal((n + 1, 2))
    Xn = np.concatenate([Fn, np.zeros((n + 1, 1))], axis=1)
    (mu, var_f), (mu1, var1) = m.predict_f(Xn), m1.predict_f(Fn)
    yscale, s2 = float(np.abs(Y).max()), max(float(var1.max()), 1.0)
    check_mean(mu.numpy(), mu1.numpy(), cond, yscale)
    check_var(var_f.numpy(), var1.numpy(), s2)
    check_var(m.predict_y(Xn)[1].numpy(), m1.predict_y(Fn)[1].numpy(), s2)
    check_var(m.predict_f(Xn, full_cov=True)[1].numpy(), m1.predict_f(Fn, full_cov=True)[1].numpy(), s2)


def test_row_order_invariance():
    """Permuting the stacked rows changes the loss by no more than check_loss's bar."""
    i = [j for j, c in enumerate(C.PARITY_CASES) if c["n"] == 200 and c["partners"] and c["layout"] == "perm"][0]
    c = C.PARITY_CASES[i]
    cond = _reference(i)[0]["cond"]
    X, Y = C.make_data(c)
    base = float(C.gpx_model(c).training_loss())
    for seed in (1, 2):
        perm = np.random.default_rng(seed).permutation(len(X))
        check_loss(float(C.gpx_model(c, data=(X[perm], Y[perm])).training_loss()), base, cond)
    order = np.argsort(X[:, c["Df"]], kind="stable")      # and sorted by asset
    check_loss(float(C.gpx_model(c, data=(X[order], Y[order])).training_loss()), base, cond)


def test_cross_asset_posterior_of_one_day():
    """predict_f(full_cov=True) at the P rows of one future day is the P × P posterior covariance
    between the assets: the reference's, symmetric, and positive semi-definite within the variance
    bar's absolute term."""
    i = [j for j, c in enumerate(C.PARITY_CASES) if c["n"] == 600 and c["P"] == 5][0]
    c = C.PARITY_CASES[i]
    cond = _reference(i)[0]["cond"]
    P = c["P"]
    day = np.random.default_rng(77).standard_normal(c["Df"])
    Xd = np.concatenate([np.tile(day, (P, 1)), np.arange(P, dtype=np.float64)[:, None]], axis=1)
    fm, fv, fc = C.oracle_values(c, [Xd])["pred"][0]
    m = C.gpx_model(c)
    mu, cov = m.predict_f(Xd, full_cov=True)
    assert mu.shape == (P, 1) and cov.shape == (1, P, P)
    cov = cov.numpy()[0]
    s2 = max(float(np.max(np.diag(fc))), 1.0)
    check_mean(mu.numpy(), fm, cond, float(np.abs(m.data[1].numpy()).max()))
    check_var(cov, fc, s2)
    check_var(cov, cov.T, s2)
    assert np.abs(fc - np.diag(np.diag(fc))).max() > 1e-3 * s2       # (the assets do co-move in this posterior)
    eig = np.linalg.eigvalsh(0.5 * (cov + cov.T))
    assert eig.min() >= -1e-10 * s2


# ---------------------------------------------------------------------------- mixed batches
def _mixed_models(ns, seed0):
    """{isotropic SE, SE-ARD, Exp x Coregion, SE x Coregion} on two feature columns + an index
    column, ragged N."""
    out = []
    for j, n in enumerate(ns):
        c = C.case([], 3, 1, n, 2, seed=seed0 + j, layout="perm")
        X, Y = C.make_data(c)
        k = [lambda: K.SquaredExponential(lengthscales=1.3, active_dims=[0, 1]),
             lambda: K.SquaredExponential(lengthscales=[0.7, 1.4], active_dims=[0, 1]),
             lambda: _set_coregion(K.Exponential(lengthscales=1.5, active_dims=[0, 1]) * K.Coregion(3, 1, active_dims=[2]),
                                   [[0.4], [-0.3], [0.5]], [0.6, 0.7, 0.8]),
             lambda: _set_coregion(K.SquaredExponential(lengthscales=1.1, active_dims=[0, 1]) * K.Coregion(3, 2, active_dims=[2]),
                                   [[0.4, -0.1], [-0.3, 0.2], [0.5, 0.3]], [0.5, 0.5, 0.5])][j % 4]()
        m = gpx.models.GPR((X, Y), kernel=k, noise_variance=1e-2)
        gpx.set_trainable(m.likelihood.variance, False)
        out.append(m)
    return out


def test_mixed_batch_fits_equal_solo_fits():
    """As tests/test_ard_gpu.py's test of the same name, with Coregion slots in the batch, and with
    equal bits asked of the solo and the batched fits: the same evaluation counts, final x and loss."""
    ns = [200, 217, 234, 251]  # (one padded size: a slot's arithmetic depends on its own data and Np)
    seq = [gpx.optimizers.Scipy().minimize(m.training_loss, m.trainable_variables, options=dict(maxiter=30))
           for m in _mixed_models(ns, 80)]
    bat = gpx.optimizers.Scipy().minimize_batch(_mixed_models(ns, 80), options=dict(maxiter=30))
    for a, b in zip(seq, bat):
        assert a.nfev == b.nfev and a.nit == b.nit
        np.testing.assert_array_equal(a.x, b.x)       # bit for bit: the final θ ...
        assert a.fun == b.fun                          # ... and the final loss


@pytest.mark.parametrize("ns", [[5, 60, 33, 64], [67, 100, 128, 90], [200, 217, 234, 251, 256, 130, 140, 150]],
                         ids=["Np64", "Np128", "Np256"])
def test_mixed_engine_call_equals_slot_by_slot_calls(ns):
    """Engine.lml_grad at fixed θ over mixed slots (plain, ARD, Coregion): every slot's bits are the
    ones it gets alone, whichever specs share the call and in whichever order; a repeated Coregion
    evaluation gives equal bits; predictions likewise."""
    models = _mixed_models(ns, 90)
    eng = Engine([m.data[0] for m in models], [m.data[1] for m in models], [m._spec for m in models])
    theta = np.stack([m.theta_row() for m in models])
    B = len(models)
    lml, grad, info = eng.lml_grad(list(range(B)), theta)
    assert not info.any()
    for b in range(B):
        for _ in range(2):  # (twice: equal bits)
            l1, g1, i1 = eng.lml_grad([b], theta)
            assert i1[b] == 0 and l1[b] == lml[b]
            np.testing.assert_array_equal(g1[b], grad[b])
    l2, g2, _ = eng.lml_grad(list(range(B))[::-1], theta)
    np.testing.assert_array_equal(l2, lml)
    np.testing.assert_array_equal(g2, grad)
    xs = [C.prediction_inputs(dict(Df=2, P=3), 9, np.random.default_rng(b)) for b in range(B)]
    m_all, v_all, _ = eng.predict(list(range(B)), theta, xs, False)
    for b in range(B):
        m1, v1, _ = eng.predict([b], theta, [xs[b]], False)
        np.testing.assert_array_equal(m1[0].cpu().numpy(), m_all[b].cpu().numpy())
        np.testing.assert_array_equal(v1[0].cpu().numpy(), v_all[b].cpu().numpy())
    assert np.all(eng.band_class(list(range(B)), theta)[[b for b in range(B) if b % 4 >= 2]] == -1)


# ---------------------------------------------------------------------------- end to end
def test_fit_learns_the_sign():
    """Three assets drawn from a known B with asset 2 moving against the others, N = 3 × 60:
    Scipy().minimize from GPflow's default start (all of B positive) against scipy's L-BFGS-B on
    the restatement from the same start: the same off-diagonal sign pattern of the fitted
    output_covariance() (the restatement's own fit separates the signs clearly,
    tests/test_coregion_api.py) and a final loss within 1e-5·|loss| (the end-to-end bar of
    SURVEY §8c)."""
    X, Y = C.sign_data()
    c = C.sign_case()
    m = C.gpx_model(c, data=(X, Y))
    res = gpx.optimizers.Scipy().minimize(m.training_loss, m.trainable_variables, options=dict(maxiter=100))
    t = C.TorchCoregion(c, data=(X, Y))
    ref = scipy.optimize.minimize(lambda u: t.loss_and_grad(u), t.u0, jac=True, method="L-BFGS-B",
                                  options=dict(maxiter=100))
    cg = m.kernel.kernels[1]
    B, B_ref = cg.output_covariance(), t.output_covariance(ref.x)
    off = ~np.eye(3, dtype=bool)
    np.testing.assert_array_equal(np.sign(B[off]), np.sign(B_ref[off]))
    assert B[0, 2] < 0 and B[1, 2] < 0 and B[0, 1] > 0
    assert abs(res.fun - ref.fun) <= 1e-5 * abs(ref.fun), (res.fun, ref.fun)


def test_stacked_assets_fit_and_joint_prediction():
    """The drop-in snippet: five ragged assets stacked, Exp × Coregion(5, 1), fitted; predict_f with
    full_cov at one day's five rows gives the [1, 5, 5] cross-asset covariance."""
    rng = np.random.default_rng(5)
    series = []
    for p, n in enumerate((63, 64, 65, 66, 67)):
        F = rng.standard_normal((n, 4))
        series.append((F, ((1.0 if p < 3 else -0.8) * np.sin(F[:, :1]) + 0.05 * rng.standard_normal((n, 1)))))
    X, Y, idx = trainer.stack_assets(series)
    k = K.Exponential(active_dims=slice(0, idx)) * K.Coregion(output_dim=5, rank=1, active_dims=[idx])
    m = gpx.models.GPR((X, Y), kernel=k, noise_variance=1e-3)
    l0 = float(m.training_loss())
    res = gpx.optimizers.Scipy().minimize(m.training_loss, m.trainable_variables, options=dict(maxiter=40))
    assert res.fun < l0 and np.isfinite(res.fun)
    X_day = np.concatenate([np.tile(rng.standard_normal(4), (5, 1)), np.arange(5.0)[:, None]], axis=1)
    mean, cov = m.predict_f(X_day, full_cov=True)
    assert mean.shape == (5, 1) and cov.shape == (1, 5, 5)
    assert np.all(np.isfinite(cov.numpy())) and np.all(np.diag(cov.numpy()[0]) > 0)
    parts = trainer.unstack_assets(m.predict_f(X)[0], X, idx)
    assert [len(p) for p in parts] == [63, 64, 65, 66, 67]


# ---------------------------------------------------------------------------- failure semantics
def test_invalid_parameters_raise_invalid_parameter_error():
    c = C.PARITY_CASES[1]
    m = C.gpx_model(c)
    cg = m.kernel.kernels[-1]
    good = float(m.training_loss())
    u = cg.kappa.unconstrained.copy()
    ub = u.copy()
    ub[1] = -1e4                                   # softplus underflows: κ_1 = 0
    cg.kappa.set_unconstrained(ub)
    with pytest.raises(N.InvalidParameterError):
        m.training_loss()
    cg.kappa.set_unconstrained(u)
    W = cg.W.value
    for bad in (np.nan, np.inf, -np.inf):
        Wb = W.copy()
        Wb[2, 0] = bad
        cg.W.assign(Wb)
        with pytest.raises(N.InvalidParameterError):
            m.training_loss()
    cg.W.assign(W)
    assert float(m.training_loss()) == good
    Wn = W.copy()
    Wn[:, 0] = [-40.0, -25.0, 0.0]                  # large negative (and zero) W: a valid θ
    cg.W.assign(Wn)
    loss, g = m.loss_and_grad_unconstrained()
    assert np.isfinite(loss) and np.all(np.isfinite(g))


def test_not_positive_definite_raises_as_the_isotropic_path_does():
    """Duplicate inputs of one asset under a kernel variance of 2^40 (W = 0, κ = 1: B = I exactly):
    the noise is below half an ulp of the diagonal, so the second pivot is exactly 0 — for the
    Coregion spec as for the isotropic one."""
    X = np.array([[1.0, 0.0], [1.0, 0.0], [3.0, 1.0]])
    ks = [_set_coregion(K.SquaredExponential(variance=2.0 ** 40, active_dims=[0]) * K.Coregion(2, 1, active_dims=[1]),
                        np.zeros((2, 1)), np.ones(2)),
          K.SquaredExponential(variance=2.0 ** 40, active_dims=[0])]
    for k in ks:
        m = gpx.models.GPR((X, np.zeros((3, 1))), kernel=k, noise_variance=2e-6)
        with pytest.raises(N.NotPositiveDefiniteError) as e:
            m.training_loss()
        assert e.value.info == 2


def test_c_abi_refusals_and_band_queries():
    """spec_error's refusals through Engine (GPX_BAD_ARG with a gpx_last_error text: GPXError, before
    any device work), and a Coregion slot is reported dense by the band queries."""
    X, Y = C.make_data(C.case([], 2, 1, 20, 1, seed=6))

    def good():
        return compile_spec(K.SquaredExponential(active_dims=[0]) * K.Coregion(2, 1, active_dims=[1]), 2)
    Engine([X], [Y], [good()])
    muts = [("exactly one input column", lambda s: (setattr(s.terms[1], "dim_count", 2), setattr(s.terms[1], "dim_start", 0))),
            ("P >= 1 and R >= 1", lambda s: setattr(s, "reserved", 1 << 8)),
            ("P >= 1 and R >= 1", lambda s: setattr(s, "reserved", 2)),
            ("one Coregion term", lambda s: (setattr(s.terms[0], "kind", N.GPX_COREGION), setattr(s.terms[0], "dim_count", 1))),
            ("GPX_SUM", lambda s: setattr(s, "combine", N.GPX_SUM)),
            ("bad kernel term", lambda s: setattr(s, "reserved", 6 | (2 << 8))),
            ("bad kernel term", lambda s: setattr(s.terms[0], "kind", N.GPX_SE | 0x200))]
    for text, mut in muts:
        s = good()
        mut(s)
        with pytest.raises(gpx.GPXError, match=text):
            Engine([X], [Y], [s])
    over = compile_spec(K.SquaredExponential(active_dims=[0]) * K.Coregion(6, 1, active_dims=[1]), 2)
    Engine([X], [Y], [over])                                            # 15 columns: accepted
    over = compile_spec(K.Coregion(3, 2, active_dims=[1]), 2)
    over.reserved, over.n_params = 5 | (2 << 8), 15                     # 10 + 5 (+ 1) = 16 columns
    with pytest.raises(gpx.GPXError, match="GPX_THETA_STRIDE - 1"):
        Engine([X], [Y], [over])
    plain = compile_spec(K.SquaredExponential(active_dims=[0]), 2)
    plain.reserved = 3
    with pytest.raises(gpx.GPXError, match="reserved must be 0"):
        Engine([X], [Y], [plain])
    # theta screening at the C ABI: NaN in W and κ = 0 are GPX_BAD_ARG, a negative W is not
    eng = Engine([X], [Y], [good()])
    th = np.ones((1, N.GPX_THETA_STRIDE))
    th[0, 2] = -2.0
    assert eng.lml_grad([0], th)[2][0] == 0
    lib = eng.lib
    for col, bad in ((2, np.nan), (4, 0.0)):
        tb = th.copy()
        tb[0, col] = bad
        act, info = np.zeros(1, dtype=np.int32), np.zeros(1, dtype=np.int32)
        lml, grad = np.zeros(1), np.zeros((1, N.GPX_THETA_STRIDE))
        dp, ip = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        rc = lib.gpx_batch_lml_grad(eng.handle, 1, act.ctypes.data_as(ip), tb.ctypes.data_as(dp),
                                    lml.ctypes.data_as(dp), grad.ctypes.data_as(dp), info.ctypes.data_as(ip),
                                    eng._stream())
        assert rc == N.GPX_BAD_ARG
    # far-apart sorted inputs: an isotropic spec is banded there, the Coregion one dense (-1)
    n = 600
    xs = np.stack([np.arange(n) * 1000.0, np.arange(n) % 2], axis=1)
    ys = np.zeros((n, 1))
    e2 = Engine([xs, xs], [ys, ys], [good(), compile_spec(K.SquaredExponential(active_dims=[0]), 2)])
    th2 = np.ones((2, N.GPX_THETA_STRIDE))
    assert e2.band_class([0, 1], th2)[0] == -1 and e2.band_width([0, 1], th2)[0] == -1
    assert e2.band_class([0, 1], th2)[1] != -1
    e3 = Engine([xs], [ys], [good()], band_storage=True)                 # band storage: the fallback slots
    l3, _, i3 = e3.lml_grad([0], th2[:1])
    l2, _, i2 = e2.lml_grad([0], th2)
    assert i3[0] == 0 and i2[0] == 0
    check_loss(l3[0], l2[0])
