"""VGP on the GPU (libgpx.so gpx_vgp_*) against the CPU restatement (tests/vgp_numpy.py).

Tolerances follow tests/test_sgpr_gpu.py's rule, not constants: per case the restatement is
evaluated by its two routes (GPflow's triangular solves; the explicit W = L⁻¹ with L = tril(K̃ Wᵀ),
as the device computes) and the spread between them — a property of the references, never of the
device result — sets the bar:

    |F_dev − F_gpflow|  <=  max(10 · |F_gpflow − F_w|,          1e-12 · |F|)
    |g_dev − g_gpflow|  <=  max(10 · max|g_gpflow − g_w|,       1e-10 · (1 + max|g|))   per block

(10x: the device sums in another order again — MFMA accumulation, wave reductions). Every case must
also have cond(K̃) <= 1e6 and resulting bars <= 1e-8·|F| and <= 1e-6·(1 + max|g|); both are asserted.

Spreads of the two routes measured on the CPU (relative to |F|; gradient blocks relative to
1 + max|g|), with cond(K̃):

    case    cond(K̃)   F         theta     lik       q_mu      q_sqrt
    tiny    1.9       0         1.5e-16   0         1.6e-16   1.2e-16
    leaf    2.9e1     0         3.8e-16   0         1.1e-16   1.6e-16
    ref     2.3e1     0         1.4e-16   3.5e-16   1.3e-16   1.3e-16
    node    3.8e4     0         4.4e-15   2.8e-15   1.7e-14   4.3e-15
    deep    2.4e2     0         1.6e-16   0         7.4e-16   7.1e-16
    gauss   1.6e1     0         7.2e-18   1.4e-16   2.9e-16   3.3e-16
    fit40   1.9e3     1.5e-16   2.8e-15   2.0e-16   6.7e-16   2.0e-15

(fit40 at its start; after 20 L-BFGS-B iterations of the restatement cond(K̃) is 5.9e3 and the
spreads stay below 5e-13.) One-column cases other than the reference's day offsets put X on a
jittered grid, and "node" lowers the Linear term's variance to 0.1: uniformly drawn points leave
near-duplicates whose eigenvalue is the jitter itself (cond 4e7 for "node" with GPflow's defaults).

The floors (1e-12, 1e-10) are therefore the bar on every case. Device errors measured on one
MI355X, as fractions of the bars: F at most 5e-4 ("node"), gradient blocks at most 3e-4 ("node",
q_mu); the fitted losses 3e-4 ("tiny") and 1e-2 ("fit40") of theirs.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

import portfoliooptgp_amd as gpx  # noqa: E402
from portfoliooptgp_amd import _native as N  # noqa: E402
from tests.test_gpu_parity import gpx_kernel, oracle_kernel  # noqa: E402
from tests.vgp_numpy import NumpyVGP  # noqa: E402

# name: N, D, family, likelihood, likelihood parameter, df, seed
CASES = {
    "tiny":  (5, 1, "se", "studentt", 0.3, 4.0, 1),            # far below one leaf, identity padding
    "leaf":  (64, 2, "se*m12", "studentt", 0.3, 4.0, 2),       # exactly one 64-leaf, no padding
    "ref":   (113, 1, "se", "studentt", 1.0, 3.0, 3),          # the reference's shape, one 128-leaf
    "node":  (130, 1, "exp+per+lin", "studentt", 0.3, 5.0, 4),  # Np = 192: a recursion node, an L21 panel
    "deep":  (257, 3, "m52", "gaussian", 0.05, 3.0, 5),        # Np = 320: two recursion levels, ragged
    "gauss": (113, 1, "se", "gaussian", 0.05, 3.0, 6),         # closed-form likelihood path
    "fit40": (40, 1, "m32", "studentt", 0.5, 3.0, 7),          # the second fit case
}
# kernel parameter overrides by position in kernel.parameters (GPflow's defaults otherwise): the
# Linear term's variance of "node", which alone would put cond(K̃) at 3e5
KPARAMS = {"node": {5: 0.1}}
PARITY = ["tiny", "leaf", "ref", "node", "deep", "gauss"]
BLOCKS = ("theta", "lik", "q_mu", "q_sqrt")


def build(name):
    """(X, Y, q, R, device kernel, oracle kernel) of a case: Y with a few 5σ outliers, a random q,
    a random lower-triangular R with its diagonal in [0.3, 1.5]."""
    n, D, fam, lik, phi, df, seed = CASES[name]
    rng = np.random.default_rng(seed)
    if name in ("ref", "gauss"):   # day offsets 0..360, as the reference's X
        X = np.sort(np.concatenate([[0, 360], rng.choice(np.arange(1, 360), n - 2, replace=False)]))
        X = X.astype(np.float64)[:, None]
        Y = np.sin(X / 40.0) + 0.1 * rng.standard_normal((n, 1))
    else:
        # (one input column: a jittered grid — near-duplicate points would leave cond(K̃) at the
        # mercy of the 1e-6 jitter)
        X = (rng.uniform(0, 10, (n, D)) if D > 1
             else (np.linspace(0, 10, n) + rng.uniform(-0.3, 0.3, n) * 10.0 / n)[:, None])
        Y = np.sin(X[:, :1]) + 0.3 * np.cos(2 * X[:, -1:]) + 0.1 * rng.standard_normal((n, 1))
    out = rng.choice(n, max(1, n // 25), replace=False)
    Y[out, 0] += 0.5 * rng.choice([-1.0, 1.0], len(out))   # 5σ of the 0.1 noise
    q = 0.5 * rng.standard_normal(n)
    R = np.tril(0.1 * rng.standard_normal((n, n)), -1) + np.diag(rng.uniform(0.3, 1.5, n))
    gk, ok = gpx_kernel(fam), oracle_kernel(fam)
    for i, v in KPARAMS.get(name, {}).items():
        gk.parameters[i].assign(v)
        ok.params()[i].value = v
    return X, Y, q, R, gk, ok


def restatement(name, state=None):
    """The case's NumpyVGP; state = (kernel parameter values, likelihood parameter, q, R) overrides
    the case's own."""
    X, Y, q, R, _, ok = build(name)
    _, _, _, lik, phi, df, _ = CASES[name]
    om = NumpyVGP(ok, X, Y, likelihood=lik, scale=phi, variance=phi, df=df)
    om.q, om.R = q, R
    if state is not None:
        kp, phi, om.q, om.R = state
        for p, v in zip(ok.params(), kp):
            p.value = float(v)
        om.lik.value = float(phi)
    return om


def bars(om):
    """The GPflow-route F and gradient blocks, and the bars from the two routes' spread."""
    Fa, ga = om.elbo_and_grads("gpflow")
    Fb, gb = om.elbo_and_grads("w")
    ga = {k: np.atleast_1d(np.asarray(ga[k], dtype=np.float64)) for k in BLOCKS}
    gb = {k: np.atleast_1d(np.asarray(gb[k], dtype=np.float64)) for k in BLOCKS}
    spreadg = {k: float(np.abs(ga[k] - gb[k]).max()) for k in BLOCKS}
    tolF = max(10.0 * abs(Fa - Fb), 1e-12 * abs(Fa))
    tolg = {k: max(10.0 * spreadg[k], 1e-10 * (1.0 + float(np.abs(ga[k]).max()))) for k in BLOCKS}
    return dict(F=Fa, g=ga, tolF=tolF, tolg=tolg, spreadF=abs(Fa - Fb), spreadg=spreadg,
                cond=float(np.linalg.cond(om.kxx())))


@functools.lru_cache(maxsize=None)
def reference(name):
    return bars(restatement(name))


def model(name, with_q=True):
    X, Y, q, R, gk, _ = build(name)
    _, _, _, lik, phi, df, _ = CASES[name]
    like = gpx.likelihoods.Gaussian(phi) if lik == "gaussian" else gpx.likelihoods.StudentT(scale=phi, df=df)
    m = gpx.models.VGP((X, Y), kernel=gk, likelihood=like)
    if with_q:
        m.q_mu.assign(q[:, None])
        m.q_sqrt.assign(R[None])
    return m


def _got(m):
    F, gth, gq, gR = m._elbo_and_grads()
    np_ = len(m.kernel.parameters)
    assert np.all(gth[np_ + 1:] == 0.0)
    assert np.all(np.triu(gR, 1) == 0.0)
    return F, {"theta": gth[:np_], "lik": gth[np_:np_ + 1], "q_mu": gq, "q_sqrt": gR}


def _compare(name, F, got, ref):
    print(f"{name}: cond={ref['cond']:.3g} F={ref['F']:.17g} dF={abs(F - ref['F']):.3g} tolF={ref['tolF']:.3g} "
          f"spreadF={ref['spreadF']:.3g}")
    errs = {k: float(np.abs(got[k] - ref["g"][k]).max()) for k in BLOCKS}
    for k in BLOCKS:
        print(f"  {k}: err={errs[k]:.3g} tol={ref['tolg'][k]:.3g} spread={ref['spreadg'][k]:.3g} "
              f"max|g|={np.abs(ref['g'][k]).max():.3g}")
    assert abs(F - ref["F"]) <= ref["tolF"], (name, F, ref["F"], ref["tolF"])
    for k in BLOCKS:
        assert errs[k] <= ref["tolg"][k], (name, k, errs[k], ref["tolg"][k])


def _assert_case_is_well_posed(name, ref):
    assert ref["cond"] <= 1e6, (name, ref["cond"])
    assert ref["tolF"] <= 1e-8 * abs(ref["F"]), (name, ref["tolF"], ref["F"])
    for k, t in ref["tolg"].items():
        assert t <= 1e-6 * (1.0 + float(np.abs(ref["g"][k]).max())), (name, k, t)


@pytest.mark.parametrize("name", PARITY)
def test_elbo_and_gradients_vs_restatement(name):
    ref = reference(name)
    _assert_case_is_well_posed(name, ref)
    F, got = _got(model(name))
    _compare(name, F, got, ref)


@pytest.mark.parametrize("name", ["ref", "node", "gauss"])
def test_predict_f_and_predict_y(name):
    """30 points, ten of them training points. Bars as tests/test_sgpr_gpu.py sets them (10x the two
    routes' spread, floor 1e-10 · (1 + max|ref|)), and the fixed ones besides: the mean within
    1e-10 · (1 + |m|), the variance within 1e-9 · (k** + the likelihood's variance)."""
    X, Y, q, R, _, ok = build(name)
    om = restatement(name)
    rng = np.random.default_rng(8)
    xs = np.concatenate([X[rng.choice(len(X), 10, replace=False)], rng.uniform(X.min() - 1, X.max() + 1, (20, 1))])
    m = model(name)
    _, _, _, lik, phi, df, _ = CASES[name]
    likvar = phi if lik == "gaussian" else phi * phi * df / (df - 2.0)
    kss = ok.K_diag(xs)[:, None]
    for fn, add in (("predict_f", 0.0), ("predict_y", likvar)):
        (mo, vo), (mw, vw) = getattr(om, fn)(xs, "gpflow"), getattr(om, fn)(xs, "w")
        mu, var = getattr(m, fn)(xs)
        assert tuple(mu.shape) == (30, 1) and tuple(var.shape) == (30, 1) and not mu.is_cuda
        for what, got, a, b in (("mean", mu.numpy(), mo, mw), ("var", var.numpy(), vo, vw)):
            tol = max(10.0 * float(np.abs(a - b).max()), 1e-10 * (1.0 + float(np.abs(a).max())))
            err = float(np.abs(got - a).max())
            print(f"{name}: {fn} {what} err={err:.3g} tol={tol:.3g}")
            assert err <= tol, (name, fn, what, err, tol)
        assert np.all(np.abs(mu.numpy() - mo) <= 1e-10 * (1.0 + np.abs(mo)))
        assert np.all(np.abs(var.numpy() - vo) <= 1e-9 * (kss + add))
    vf, vy = m.predict_f(xs)[1].numpy(), m.predict_y(xs)[1].numpy()
    np.testing.assert_allclose(vy - vf, likvar, rtol=1e-9)
    mu0, var0 = m.predict_f(np.zeros((0, 1)))  # empty Xnew: empty outputs
    assert tuple(mu0.shape) == (0, 1) and tuple(var0.shape) == (0, 1)


@pytest.mark.parametrize("name", ["tiny", "fit40"])
def test_scipy_fit_lowers_the_loss_and_matches_restatement(name):
    """The reference's cell: Scipy().minimize(model.training_loss, model.trainable_variables), from
    GPflow's initial q_mu = 0, q_sqrt = I. The loss returned is below the start, and the restatement
    at the returned parameters reproduces it within the bar of that state."""
    m = model(name, with_q=False)
    start = float(m.training_loss())
    res = gpx.optimizers.Scipy().minimize(m.training_loss, m.trainable_variables, options=dict(maxiter=20))
    assert res.fun < start, (name, res.fun, start)
    om = restatement(name, ([p.value for p in m.kernel.parameters], m._lik_param.value,
                            m.q_mu.value.reshape(-1), m.q_sqrt.value[0]))
    ref = bars(om)
    _assert_case_is_well_posed(name, ref)
    print(f"{name}: start {start:.12g} fitted {res.fun:.17g} in {res.nit} its; restatement {-ref['F']:.17g} "
          f"tolF={ref['tolF']:.3g}")
    assert abs(res.fun + ref["F"]) <= ref["tolF"], (name, res.fun, -ref["F"], ref["tolF"])
    assert float(m.training_loss()) == res.fun


def test_second_evaluation_equals_fresh_model():
    """No stale padding or workspace: after one evaluation, a second one on the same model with
    another q, R and θ gives the bits a fresh model gives."""
    name = "node"
    n = CASES[name][0]
    rng = np.random.default_rng(11)
    q2 = rng.standard_normal(n)
    R2 = np.tril(0.3 * rng.standard_normal((n, n)), -1) + np.diag(rng.uniform(0.3, 1.5, n))

    def move(m):
        m.q_mu.assign(q2[:, None])
        m.q_sqrt.assign(R2[None])
        for p in m.kernel.parameters:
            p.assign(p.value * 1.3)
        m.likelihood.scale.assign(0.7)

    used = model(name)
    used._elbo_and_grads()
    used.predict_y(build(name)[0][:7])
    move(used)
    fresh = model(name)
    move(fresh)
    Fu, gu = _got(used)
    Ff, gf = _got(fresh)
    assert Fu == Ff
    for k in BLOCKS:
        np.testing.assert_array_equal(gu[k], gf[k])
    om = restatement(name, ([p.value for p in fresh.kernel.parameters], 0.7, q2, R2))
    _compare(name + "/moved", Ff, gf, bars(om))


def test_errors():
    m = model("tiny")
    eng = m.engine()
    th, q, R = m._state()
    bad = th.copy()
    bad[len(m.kernel.parameters)] = -1.0
    with pytest.raises(gpx.GPXError, match=r"\(2\)"):       # GPX_BAD_ARG through the engine
        eng.elbo_grad(bad, q, R)
    R0 = R.copy()
    R0[2, 2] = 0.0
    with pytest.raises(gpx.GPXError, match="zero diagonal"):
        eng.elbo_grad(th, q, R0)
    qn = q.copy()
    qn[1] = np.nan
    with pytest.raises(gpx.GPXError, match="finite"):
        eng.predict(th, qn, R, np.zeros((3, 1)), False)
    m.likelihood.scale.set_unconstrained(-1e4)               # softplus underflows to scale = 0
    with pytest.raises(gpx.InvalidParameterError):
        m.training_loss()
    with pytest.raises(ValueError):
        gpx.likelihoods.StudentT(df=2.0)                      # refused at construction
    assert N.GPX_BAD_ARG == 2
    F, _ = _got(model("tiny"))                                # and the engine still evaluates
    assert np.isfinite(F)


def test_not_positive_definite_reports_the_pivot():
    """Duplicate inputs under a kernel variance of 2^40: the 1e-6 jitter is below half an ulp of
    the diagonal, so the second pivot is exactly 0."""
    X = np.array([[1.0], [1.0], [3.0]])
    k = gpx.kernels.SquaredExponential(variance=2.0 ** 40)
    m = gpx.models.VGP((X, np.zeros((3, 1))), kernel=k, likelihood=gpx.likelihoods.StudentT())
    with pytest.raises(gpx.NotPositiveDefiniteError) as e:
        m.training_loss()
    assert e.value.info == 2
    with pytest.raises(gpx.NotPositiveDefiniteError):
        m.predict_f(X)
