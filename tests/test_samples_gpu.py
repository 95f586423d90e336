"""GPR posterior sampling on the GPU (gpx_sample_mvn, gpx_batch_predict_samples, models.GPR.
predict_f_samples) against the numpy restatement of tests/sample_numpy.py.

Shapes: M over every block boundary of the factorisation (64) and of its 16-column steps, S over the
product GEMM's 64-row padding. Every input's cond(cov + 1e-6·I), computed from the oracle, is asserted
<= 1e8, so an ill-conditioned input cannot pass as a well-conditioned one.

How the three layers of the check fit together. The device's draw is out = mean + P with P the
product L·white. The bounds below are stated on P — the sampler called with a zero mean on the
device's own predict_f(full_cov=True) covariance — because that is where they can hold: the final
addition rounds once to ulp(|mean + P|), which exceeds a bound proportional to ‖L‖·‖white‖ as soon as
|mean| >> ‖L‖ (M = 1, 2 here: L ~ 1e-3, mean ~ 1), whatever the implementation. The model path is then
held to mean + P *bit for bit*, which together with the bound on P is the statement on out.
  factor   white = I: P = L exactly. L lower-triangular, positive diagonal,
           |LLᵀ − A|_ij <= 4·(M+1)·u·sqrt(A_ii A_jj), A = device covariance + jitter (Higham's
           componentwise bound; factor 4 for the MFMA summation order and the fp64 check product).
  samples  |P − white·L_refᵀ|_inf <= 2·κ₂(A)·(M+1)·u·‖L‖_F·‖white_s‖₂ per sample, L_ref LAPACK's.
  oracle   the same plus the existing full_cov parity tolerance on the covariance,
           E_ij = 1e-5·|cov_ij| + 1e-10·σ²_max (tests/test_gpu_parity.py:93-96 check_var, applied
           elementwise to full_cov by tests/test_coregion_gpu.py:73), through the first-order bound
           ‖ΔL‖_F <= ‖L‖₂·‖L⁻¹‖₂²·‖E‖_F/√2, times ‖white_s‖₂, plus check_mean's tolerance (:87-90).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import portfoliooptgp_amd as gpx  # noqa: E402
from oracle import gp_oracle as O  # noqa: E402
from portfoliooptgp_amd import _native as N  # noqa: E402
from portfoliooptgp_amd import engine as E  # noqa: E402
from portfoliooptgp_amd import mean_functions as MF  # noqa: E402
from portfoliooptgp_amd import trainer  # noqa: E402
from portfoliooptgp_amd.kernels import compile_spec  # noqa: E402
from tests import coregion_numpy as C  # noqa: E402
from tests import sample_numpy as SN  # noqa: E402
from tests.sgpr_numpy import NumpySGPR  # noqa: E402

K = gpx.kernels
DEV = "cuda:0"
U, JIT = SN.U, SN.JITTER
ARD_ELL = np.array([1.5, 2.5, 4.0])
CG_W, CG_KAPPA = C.mixed_sign_W(3, 1, 5), np.array([0.3, 0.5, 0.7])


# --------------------------------------------------------------------------------- the models
def _ard_data():
    rng = np.random.default_rng(11)
    X = rng.uniform(0, 10, (SN.N_TRAIN, 3))
    return X, np.sin(X[:, :1]) + 0.3 * X[:, 1:2] * np.cos(X[:, 2:3])


def _coreg_data():
    days = np.arange(20.0)
    X = np.concatenate([np.stack([days, np.full(20, float(p))], 1) for p in range(3)])
    return X, np.concatenate([np.sin(0.3 * days + p)[:, None] for p in range(3)])


def _coreg_xs(M):
    H = M // 3
    d = np.linspace(20, 20 + H / 2, H)
    return np.concatenate([np.stack([d, np.full(H, float(p))], 1) for p in range(3)])


@functools.lru_cache(maxsize=None)
def _case(name):
    """(gpx model, oracle model, M -> Xs for the model, Xs -> the oracle's inputs)"""
    ident = lambda x: x  # noqa: E731
    if name in ("se", "lin"):
        x, y = SN.train_data()
        mf = MF.Linear(A=[[0.02]], b=[-0.5]) if name == "lin" else None
        m = gpx.models.GPR((x, y), kernel=K.SquaredExponential(lengthscales=5.0), noise_variance=1e-5, mean_function=mf)
        return m, SN.se_oracle(), SN.xs_for, ident   # (a mean function does not change the covariance)
    if name == "m52":
        x, y = SN.train_data()
        return (gpx.models.GPR((x, y), kernel=K.Matern52(lengthscales=3.0), noise_variance=1e-3), SN.matern_oracle(),
                SN.xs_for, ident)
    if name == "ard":
        X, y = _ard_data()
        m = gpx.models.GPR((X, y), kernel=K.SquaredExponential(lengthscales=ARD_ELL, variance=1.3), noise_variance=1e-3)
        om = O.OGPR(X / ARD_ELL, y, O.OSquaredExponential(variance=1.3, lengthscales=1.0), noise_variance=1e-3)
        return m, om, lambda M: np.random.default_rng(100 + M).uniform(0, 10, (M, 3)), lambda xs: xs / ARD_ELL
    assert name == "coreg"
    X, y = _coreg_data()
    cg = K.Coregion(3, 1, active_dims=[1])
    cg.W.assign(CG_W)
    cg.kappa.assign(CG_KAPPA)
    m = gpx.models.GPR((X, y), kernel=K.SquaredExponential(lengthscales=5.0, active_dims=[0]) * cg, noise_variance=1e-3)
    kern = O.OProduct([O.OSquaredExponential(lengthscales=5.0, active_dims=[0]), C.OCoregion(CG_W, CG_KAPPA, 1)])
    return m, O.OGPR(X, y, kern, noise_variance=1e-3), _coreg_xs, ident


@functools.lru_cache(maxsize=None)
def _post(name, M):
    """Computed once per (model, M), shared, never modified: Xs, the oracle's mean / covariance and
    cond(cov + jitter·I) (asserted), the device's predict_f(full_cov=True) and A = its cov + jitter·I."""
    m, om, xs_of, to_oracle = _case(name)
    xs = xs_of(M)
    mo, co = om.predict_f(to_oracle(xs), full_cov=True)
    cond = float(np.linalg.cond(co + JIT * np.eye(M)))
    assert cond <= 1e8, (name, M, cond)
    md, cd = m.predict_f(torch.as_tensor(xs, device=DEV), full_cov=True)
    cov = cd[0].cpu().numpy()
    return dict(xs=xs, mean_o=mo[:, 0], cov_o=co, cond=cond, mean_d=md[:, 0].cpu().numpy(), cov_d_t=cd[0].contiguous(),
                A=cov + JIT * np.eye(M))


def _sampler(cov_t, white):
    """The sampler alone, zero mean, on one device covariance: white [S, M] -> P [S, M] (numpy)."""
    M = cov_t.shape[0]
    out = E.sample_mvn(torch.zeros(M, dtype=torch.float64, device=DEV), cov_t, torch.as_tensor(white, device=DEV), JIT)
    return out.cpu().numpy()


def _check_factor(A, L, tag):
    M = A.shape[0]
    assert np.all(np.triu(L, 1) == 0.0), tag
    assert np.all(np.diag(L) > 0.0), tag
    res, bound = np.abs(L @ L.T - A), SN.factor_bound(A, 4.0)
    print(f"{tag}: max residual / ((M+1)·u·sqrt(A_ii A_jj)) = {float((res / SN.factor_bound(A)).max()):.3f}")
    assert np.all(res <= bound), (tag, float((res / bound).max()))


MODEL_MS = ([("se", M) for M in SN.MS] + [("m52", M) for M in SN.MS] + [("ard", M) for M in (17, 65, 129, 200)]
            + [("coreg", M) for M in (15, 66, 129)] + [("lin", M) for M in (17, 65)])


@pytest.mark.parametrize("name,M", MODEL_MS, ids=[f"{n}-M{M}" for n, M in MODEL_MS])
def test_factor_meets_the_componentwise_bound(name, M):
    p = _post(name, M)
    L = _sampler(p["cov_d_t"], np.eye(M)).T
    _check_factor(p["A"], L, f"{name} M={M}")


@pytest.mark.parametrize("name,M", MODEL_MS, ids=[f"{n}-M{M}" for n, M in MODEL_MS])
def test_samples_against_the_restatement_on_the_device_covariance(name, M):
    """P within the perturbation bound of white·L_refᵀ, and the model's predict_f_samples equal to
    (device mean) + P bit for bit. S cycles through SS over the cases, so every S meets several M."""
    p = _post(name, M)
    S = SN.SS[(SN.MS.index(M) if M in SN.MS else M) % len(SN.SS)]
    white = np.random.default_rng(1000 + M).standard_normal((S, M))
    P = _sampler(p["cov_d_t"], white)
    Lr = SN.chol_lapack(p["A"])
    err, bound = np.abs(P - white @ Lr.T).max(axis=1), SN.sample_bound(p["A"], Lr, white)
    print(f"{name} M={M} S={S}: max err/bound = {float((err / bound).max()):.3g} (bound {float(bound.max()):.3g})")
    assert np.all(err <= bound), (name, M, S, float((err / bound).max()))
    m = _case(name)[0]
    out = m.predict_f_samples(torch.as_tensor(p["xs"], device=DEV), S, white=white[:, :, None])
    assert tuple(out.shape) == (S, M, 1) and out.is_cuda
    np.testing.assert_array_equal(out[:, :, 0].cpu().numpy(), p["mean_d"][None, :] + P)


@pytest.mark.parametrize("name,M", [("se", 17), ("se", 129), ("m52", 65), ("m52", 200), ("ard", 65), ("coreg", 66)])
def test_end_to_end_against_the_oracle(name, M):
    p = _post(name, M)
    m, om = _case(name)[:2]
    S = 3
    white = np.random.default_rng(2000 + M).standard_normal((S, M))
    ref = SN.sample_mvn(p["mean_o"], p["cov_o"], white)
    out = m.predict_f_samples(p["xs"], S, white=white[:, :, None])
    assert not out.is_cuda   # (a host Xnew: host output, as predict_f)
    Ao = p["cov_o"] + JIT * np.eye(M)
    Lo = SN.chol_lapack(Ao)
    Ecov = 1e-5 * np.abs(p["cov_o"]) + 1e-10 * max(float(np.diag(p["cov_o"]).max()), 1.0)
    dL = np.linalg.norm(Lo, 2) * np.linalg.norm(np.linalg.inv(Lo), 2) ** 2 * np.linalg.norm(Ecov) / np.sqrt(2.0)
    yscale = float(np.abs(om.Y).max())
    mean_tol = 1e-6 * np.abs(p["mean_o"]).max() + 1e-14 * float(np.linalg.cond(om._Ky())) * max(1.0, yscale)
    wn = np.linalg.norm(white, axis=1)
    bound = SN.sample_bound(Ao, Lo, white) + dL * wn + mean_tol
    err = np.abs(out[:, :, 0].numpy() - ref).max(axis=1)
    print(f"{name} M={M}: end-to-end err {float(err.max()):.3g}, bound {float(bound.min()):.3g}")
    assert np.all(err <= bound), (name, M, err, bound)


def test_marginal_form():
    """full_cov=False: mean + sqrt(var)·white from the device's predict_f, no jitter."""
    m = _case("m52")[0]
    xs = torch.as_tensor(SN.xs_for(65), device=DEV)
    white = torch.as_tensor(np.random.default_rng(3).standard_normal((4, 65, 1)), device=DEV)
    mean, var = m.predict_f(xs)
    out = m.predict_f_samples(xs, 4, full_cov=False, white=white)
    assert tuple(out.shape) == (4, 65, 1)
    np.testing.assert_allclose(out.cpu().numpy(), (mean + torch.sqrt(var) * white).cpu().numpy(), rtol=1e-14, atol=0)
    one = m.predict_f_samples(xs, full_cov=False, white=white[0])
    np.testing.assert_array_equal(one.cpu().numpy(), out[0].cpu().numpy())


# ------------------------------------------------------------------------------ band storage
def test_band_storage_batch_through_its_shadow_slots():
    """A band-storage batch (N = 512: its smallest shape) predicts new inputs on its dense fallback
    slots; the sampler follows there. Factor and samples as above, on that batch's own covariance."""
    n = 512
    x = np.arange(n, dtype=np.float64)[:, None]
    y = O.synthetic_series(n, seed=3)[1]
    spec = compile_spec(K.SquaredExponential(), 1)
    eng = E.Engine([x, x], [y, y], [spec, spec], band_storage=True)
    om = O.OGPR(x, y, O.OSquaredExponential(lengthscales=1.0), noise_variance=1e-5)
    th = np.ones((2, N.GPX_THETA_STRIDE))
    th[:, :3] = (1.0, 1.0, 1e-5)
    for M, S in ((17, 3), (65, 17)):
        xs = SN.xs_for(M)
        assert np.linalg.cond(om.predict_f(xs, full_cov=True)[1] + JIT * np.eye(M)) <= 1e8
        white = np.random.default_rng(M).standard_normal((S, M))
        means, covs, _ = eng.predict([1], th, [xs], False, full_cov=True)
        A = covs[0].cpu().numpy() + JIT * np.eye(M)
        _, eye_out, _ = eng.predict_samples([1], th, [xs], [np.eye(M)], JIT)
        L = (eye_out[0].cpu().numpy() - means[0].cpu().numpy()[None, :]).T
        # (mean + L − mean rounds at ulp(mean): the sharp factor check runs on the sampler alone)
        _check_factor(A, _sampler(covs[0].contiguous(), np.eye(M)).T, f"band M={M}")
        np.testing.assert_allclose(L, _sampler(covs[0].contiguous(), np.eye(M)).T, rtol=0,
                                   atol=4 * U * float(np.abs(means[0].cpu().numpy()).max() + np.abs(L).max()))
        mm, out, info = eng.predict_samples([1], th, [xs], [white], JIT)
        assert info[1] == 0
        np.testing.assert_array_equal(mm[0].cpu().numpy(), means[0].cpu().numpy())
        np.testing.assert_array_equal(out[0].cpu().numpy(),
                                      means[0].cpu().numpy()[None, :] + _sampler(covs[0].contiguous(), white))


# ------------------------------------------------------------------------------- invariances
def test_batch_equals_solo_bit_for_bit():
    """Three models of N = (89, 19, 5) on one engine, N* = (30, 4, 1), S = 5: predict_f_samples_batch
    (one device pass, ragged N* padded) equals each model's own predict_f_samples call."""
    ns, ms, S = (89, 19, 5), (30, 4, 1), 5
    data = [(np.arange(n, dtype=np.float64)[:, None], O.synthetic_series(n, seed=20 + n)[1]) for n in ns]
    models = [gpx.models.GPR(d, kernel=K.SquaredExponential(lengthscales=4.0 + i), noise_variance=1e-4)
              for i, d in enumerate(data)]
    eng = E.Engine([d[0] for d in data], [d[1] for d in data], [mm._spec for mm in models])
    for i, mm in enumerate(models):
        mm._attach(eng, i)
    rng = np.random.default_rng(9)
    xnews = [np.linspace(1.0, n + 2.0, M)[:, None] for n, M in zip(ns, ms)]
    whites = [rng.standard_normal((S, M, 1)) for M in ms]
    batch = gpx.models.predict_f_samples_batch(models, xnews, S, whites=whites)
    for mm, xn, w, got in zip(models, xnews, whites, batch):
        solo = mm.predict_f_samples(xn, S, white=w)
        assert tuple(got.shape) == (S, len(xn), 1)
        np.testing.assert_array_equal(got.numpy(), solo.numpy())
    # models without a shared engine are predicted one by one, to the same draws as their own calls
    loose = [gpx.models.GPR(d, kernel=K.SquaredExponential(lengthscales=4.0 + i), noise_variance=1e-4)
             for i, d in enumerate(data)]
    for got, mm, xn, w in zip(gpx.models.predict_f_samples_batch(loose, xnews, S, whites=whites), loose, xnews, whites):
        np.testing.assert_array_equal(got.numpy(), mm.predict_f_samples(xn, S, white=w).numpy())


@pytest.mark.parametrize("M", [17, 129])
def test_sample_s_does_not_depend_on_S(M):
    p = _post("se", M)
    white = np.random.default_rng(4).standard_normal((17, M))
    np.testing.assert_array_equal(_sampler(p["cov_d_t"], white)[:3], _sampler(p["cov_d_t"], white[:3]))
    m = _case("se")[0]
    xs = torch.as_tensor(p["xs"], device=DEV)
    a = m.predict_f_samples(xs, 17, white=white[:, :, None])
    b = m.predict_f_samples(xs, 3, white=white[:3, :, None])
    np.testing.assert_array_equal(a[:3].cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("M", [17, 129, 200])
def test_a_problem_alone_equals_itself_inside_a_batch(M):
    """gpx_sample_mvn at B = 1 against the same problem at position 2 of B = 3 (its neighbours: the
    Matern52 posterior and a scaled identity, so the call's tile choice and contents differ)."""
    p, q = _post("se", M), _post("m52", M)
    rng = np.random.default_rng(6)
    mean = torch.as_tensor(rng.standard_normal((3, M)), device=DEV)
    white = torch.as_tensor(rng.standard_normal((3, 5, M)), device=DEV)
    cov = torch.stack([q["cov_d_t"], 2.0 * torch.eye(M, dtype=torch.float64, device=DEV), p["cov_d_t"]])
    three = E.sample_mvn(mean, cov, white, JIT)
    alone = E.sample_mvn(mean[2:], cov[2:], white[2:], JIT)
    np.testing.assert_array_equal(three[2].cpu().numpy(), alone[0].cpu().numpy())


def test_the_gemm_tile_choice_does_not_change_a_problem():
    """B = 86, M = 384, S = 128: with that many problems the launcher gives the trailing update of
    the second block step (256 rows) and the product GEMM 128-tiles, alone they take 64-tiles. A
    128-tile trailing update writes its diagonal tiles whole, upper 64-block included, which the step
    kernel zeroes again before the product reads it. Problems 0 and 85 equal their own B = 1 calls."""
    B, M, S = 86, 384, 128
    rng = np.random.default_rng(21)
    G = rng.standard_normal((M, M))
    cov1 = torch.as_tensor(G @ G.T / M + np.eye(M), device=DEV)
    cov = cov1.expand(B, M, M).contiguous()
    mean = torch.as_tensor(rng.standard_normal((B, M)), device=DEV)
    white = torch.as_tensor(rng.standard_normal((B, S, M)), device=DEV)
    out = E.sample_mvn(mean, cov, white, JIT)
    for b in (0, 85):
        alone = E.sample_mvn(mean[b], cov1, white[b], JIT)
        np.testing.assert_array_equal(out[b].cpu().numpy(), alone.cpu().numpy())
    A = cov1.cpu().numpy() + JIT * np.eye(M)
    w, Lr = white[85].cpu().numpy(), SN.chol_lapack(A)
    ref = mean[85].cpu().numpy()[None, :] + w @ Lr.T
    tol = SN.sample_bound(A, Lr, w)[:, None] + 2 * U * np.abs(ref)   # (+ the final addition's rounding, per side)
    assert np.all(np.abs(out[85].cpu().numpy() - ref) <= tol)


# ------------------------------------------------------------------------------------ not PD
def test_not_pd_in_the_middle_of_a_batch():
    """B = 3, the middle matrix [[1, 2], [2, 1]] padded to M = 17 by an identity, jitter 0: GPX_NOT_PD,
    info = (0, 2, 0), the outer problems correct, the failed one's rows not written."""
    M, S = 17, 4
    rng = np.random.default_rng(8)
    G = rng.standard_normal((2, M, M))
    covs = np.stack([G[0] @ G[0].T + M * np.eye(M), np.eye(M), G[1] @ G[1].T + M * np.eye(M)])
    covs[1, 0, 1] = covs[1, 1, 0] = 2.0
    mean, white = rng.standard_normal((3, M)), rng.standard_normal((3, S, M))
    t = lambda a: torch.as_tensor(a, device=DEV)  # noqa: E731
    mean_t, cov_t, white_t = t(mean), t(covs), t(white)
    out = torch.full((3, S, M), -777.0, dtype=torch.float64, device=DEV)
    info = np.full(3, -1, dtype=np.int32)
    ctx = N.Context.get(0)
    vp = lambda x: ctypes.c_void_p(x.data_ptr())  # noqa: E731
    torch.cuda.synchronize()
    rc = ctx.lib.gpx_sample_mvn(ctx.handle, 3, M, S, vp(mean_t), vp(cov_t), vp(white_t), 0.0, vp(out),
                                info.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None)
    assert rc == N.GPX_NOT_PD and "positive definite" in ctx.last_error()
    assert info.tolist() == [0, 2, 0]
    got = out.cpu().numpy()
    assert np.all(got[1] == -777.0)
    for b in (0, 2):
        ref = SN.sample_mvn(mean[b], covs[b], white[b], jitter=0.0)
        L = SN.chol_lapack(covs[b])
        # (here |mean| ~ ‖L‖: the final addition's one rounding per side, 2·u·|ref|, is added)
        tol = SN.sample_bound(covs[b], L, white[b])[:, None] + 2 * U * np.abs(ref)
        assert np.all(np.abs(got[b] - ref) <= tol), b
    with pytest.raises(gpx.NotPositiveDefiniteError) as e:
        E.sample_mvn(mean_t, cov_t, white_t, 0.0)
    assert e.value.info.tolist() == [0, 2, 0]


def test_bad_arguments_are_refused_with_a_message():
    ctx = N.Context.get(0)
    buf = torch.zeros(64, dtype=torch.float64, device=DEV)
    info = np.zeros(1, dtype=np.int32)
    ip = info.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    p = ctypes.c_void_p(buf.data_ptr())
    lim = E.sample_limits()
    for args in ((1, 0, 1, 1e-6), (1, 2, 0, 1e-6), (1, lim + 1, 1, 1e-6), (1, 2, 2, -1.0), (1, 2, 2, float("inf"))):
        B, M, S, jit = args
        assert ctx.lib.gpx_sample_mvn(ctx.handle, B, M, S, p, p, p, jit, p, ip, None) == N.GPX_BAD_ARG, args
        assert ctx.last_error()
    assert ctx.lib.gpx_sample_mvn(ctx.handle, 1, 2, 2, None, p, p, 1e-6, p, ip, None) == N.GPX_BAD_ARG
    m = _case("se")[0]
    eng, b = m.engine()
    th = np.ones((eng.B, N.GPX_THETA_STRIDE))
    th[b] = m.theta_row()
    act = np.asarray([b], dtype=np.int32)
    call = lambda M, S, jit, w=p: eng.lib.gpx_batch_predict_samples(  # noqa: E731
        eng.handle, 1, act.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), th.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
        p, M, S, w, jit, p, p, ip, None)
    for M, S, jit in ((0, 1, 1e-6), (2, 0, 1e-6), (lim + 1, 1, 1e-6), (2, 2, -1e-6), (2, 2, float("nan"))):
        assert call(M, S, jit) == N.GPX_BAD_ARG, (M, S, jit)
        assert eng.ctx.last_error()
    assert call(2, 2, 1e-6, None) == N.GPX_BAD_ARG


def test_a_failed_posterior_factor_raises_naming_the_posterior_covariance():
    """Forty copies of one prediction point and jitter = 0: the posterior covariance has rank one."""
    m = _case("se")[0]
    xs = np.full((40, 1), 83.3)
    with pytest.raises(gpx.NotPositiveDefiniteError, match="posterior covariance") as e:
        m.predict_f_samples(xs, 2, white=np.ones((2, 40, 1)), jitter=0.0)
    assert e.value.info is not None and np.count_nonzero(e.value.info) == 1
    out = m.predict_f_samples(xs, 2, white=np.ones((2, 40, 1)))   # GPflow's default jitter: fine
    assert np.all(np.isfinite(out.numpy()))


# ----------------------------------------------------- shapes, placement, asset paths, log density
def test_shapes_and_placement():
    m = _case("m52")[0]
    xs = SN.xs_for(15)
    g = torch.Generator(device=DEV).manual_seed(1)
    one = m.predict_f_samples(xs)
    assert tuple(one.shape) == (15, 1) and not one.is_cuda
    many = m.predict_f_samples(torch.as_tensor(xs, device=DEV), 6, generator=g)
    assert tuple(many.shape) == (6, 15, 1) and many.is_cuda
    g2 = torch.Generator(device=DEV).manual_seed(1)
    again = m.predict_f_samples(torch.as_tensor(xs, device=DEV), 6, generator=g2)
    np.testing.assert_array_equal(many.cpu().numpy(), again.cpu().numpy())
    w = np.random.default_rng(2).standard_normal((15, 1))
    np.testing.assert_array_equal(m.predict_f_samples(xs, white=w).numpy(),
                                  m.predict_f_samples(xs, 1, white=w[None])[0].numpy())


def test_sample_asset_paths_regroups_the_joint_draws():
    m = _case("coreg")[0]
    H, S = 5, 4
    d = np.linspace(20, 22, H)
    series = [(d[:, None], np.zeros((H, 1))) for _ in range(3)]
    xa, _, idx = trainer.stack_assets(series)
    white = np.random.default_rng(12).standard_normal((S, 3 * H, 1))
    paths = trainer.sample_asset_paths(m, xa, idx, S, white=white)
    flat = m.predict_f_samples(xa, S, white=white)
    assert tuple(paths.shape) == (S, H, 3)
    for s in range(S):
        for p_, col in enumerate(trainer.unstack_assets(flat[s].numpy(), xa, idx)):
            np.testing.assert_array_equal(paths[s, :, p_].numpy(), col[:, 0])
    # any row order of Xnew: grouped by the index column, rows in their stacked order
    perm = np.random.default_rng(13).permutation(3 * H)
    shuffled = trainer.sample_asset_paths(m, xa[perm], idx, S, white=white)
    flat2 = m.predict_f_samples(xa[perm], S, white=white)
    for p_, col in enumerate(trainer.unstack_assets(flat2[0].numpy(), xa[perm], idx)):
        np.testing.assert_array_equal(shuffled[0, :, p_].numpy(), col[:, 0])


def _log_density(y, mean, var):
    return (-0.5 * (np.log(2 * np.pi) + np.log(var) + (y - mean) ** 2 / var))[:, 0]


def _density_tol(y, mean, var, dm, dv):
    """first-order propagation of a mean error dm and a variance error dv into the log density"""
    r = np.abs(y - mean)
    return (0.5 * dv / var + r * dm / var + 0.5 * r ** 2 * dv / var ** 2)[:, 0]


def test_predict_log_density_gpr_and_sgpr():
    m, om = _case("m52")[:2]
    xs = SN.xs_for(30)
    ys = np.random.default_rng(14).standard_normal((30, 1))
    mo, vo = om.predict_y(xs)
    got = m.predict_log_density((xs, ys))
    assert tuple(got.shape) == (30,) and not got.is_cuda
    # predict_y's parity tolerances (tests/test_gpu_parity.py:87-96 check_mean / check_var)
    dm = 1e-6 * np.abs(mo).max() + 1e-14 * float(np.linalg.cond(om._Ky())) * max(1.0, float(np.abs(om.Y).max()))
    dv = 1e-5 * np.abs(vo) + 1e-10 * max(float(vo.max()), 1.0)
    ref = _log_density(ys, mo, vo)
    assert np.all(np.abs(got.numpy() - ref) <= _density_tol(ys, mo, vo, dm, dv) + 8 * U * np.abs(ref))
    # SGPR (the smoke test's model): tolerances as tests/test_sgpr_gpu.py:146-150 sets them
    rng = np.random.default_rng(3)
    X = rng.uniform(0, 10, (200, 1))
    Y = np.sin(X) + 0.1 * rng.standard_normal((200, 1))
    Z = np.linspace(0, 10, 10)[:, None]
    sg = gpx.models.SGPR((X, Y), kernel=K.SquaredExponential(), inducing_variable=Z, noise_variance=0.1, device=0)
    osg = NumpySGPR(O.OSquaredExponential(), X, Y, Z, noise_variance=0.1)
    xn = rng.uniform(-1, 11, (50, 1))
    yn = np.sin(xn) + 0.3 * rng.standard_normal((50, 1))
    (ma, va), (mb, vb) = osg.predict_y(xn, "gpflow"), osg.predict_y(xn, "w")
    ma, va = np.asarray(ma).reshape(-1, 1), np.asarray(va).reshape(-1, 1)
    tol = lambda a, b: max(10.0 * float(np.abs(a - np.asarray(b).reshape(-1, 1)).max()),  # noqa: E731
                           1e-10 * (1.0 + float(np.abs(a).max())))
    got = sg.predict_log_density((xn, yn))
    ref = _log_density(yn, ma, va)
    assert tuple(got.shape) == (50,)
    assert np.all(np.abs(got.numpy() - ref) <= _density_tol(yn, ma, va, tol(ma, mb), tol(va, vb)) + 8 * U * np.abs(ref))
