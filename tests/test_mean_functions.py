"""GPR mean functions (Constant, Linear, Polynomial): the Python surface, the θ-row layout, the
transform-coded host helpers, and the numpy reference the GPU tests compare against. No GPU here.

The reference (``ref_eval``): with r = y − m(X; β), the oracle's GPR on r gives logML and the kernel
and noise gradients, and ∂logML/∂β = Φᵀα with α = (K + σn²I)⁻¹ r from scipy's cho_solve. It is
checked below against central differences of the oracle's logML (N = 60, ``Polynomial(2)`` on raw
day offsets, whose three gradient components differ by orders of magnitude): 1e-7 relative per
component.
"""
import ctypes

import numpy as np
import pytest
import scipy.linalg as sla

import portfoliooptgp_amd as gpx
from portfoliooptgp_amd import _native as N
from oracle import gp_oracle as O

K = gpx.kernels
MF = gpx.mean_functions


# ------------------------------------------------------------------ the reference ---------
def mean_basis(kind, X, degree=0):
    """Φ [N, n_coef] with m(X; β) = Φβ, β in the θ-row order (Constant [c]; Linear [A.., b];
    Polynomial [w_0 .. w_degree])."""
    X = np.asarray(X, dtype=np.float64).reshape(len(X), -1)
    one = np.ones((X.shape[0], 1))
    if kind == "constant":
        return one
    if kind == "linear":
        return np.hstack([X, one])
    if kind == "polynomial":
        return np.hstack([X[:, :1] ** k for k in range(degree + 1)])
    raise ValueError(kind)


def ref_eval(X, y, okernel, noise, kind, beta, degree=0, noise_trainable=True):
    """(logML, ∂(−logML)/∂u of the kernel and noise variables, ∂logML/∂β, α, Φ)."""
    Phi = mean_basis(kind, X, degree)
    r = np.asarray(y, dtype=np.float64).reshape(-1) - Phi @ np.asarray(beta, dtype=np.float64)
    om = O.OGPR(X, r, okernel, noise_variance=noise)
    om.noise.trainable = noise_trainable
    loss, g_u = om.loss_and_grad_u()
    alpha = sla.cho_solve(sla.cho_factor(om._Ky(), lower=True), r)
    return -loss, g_u, Phi.T @ alpha, alpha, Phi


def series(n, seed=3):
    """Raw day offsets 0..n-1 and a series with a quadratic trend on top of the oracle's draw."""
    x = np.arange(n, dtype=np.float64)[:, None]
    y = O.synthetic_series(n, seed=seed)[1].reshape(-1)
    t = x[:, 0] / n
    return x, y + 0.8 - 1.5 * t + 2.0 * t * t


def make_mean(kind, beta, degree=0):
    beta = np.asarray(beta, dtype=np.float64)
    if kind == "constant":
        return MF.Constant(beta)
    if kind == "linear":
        return MF.Linear(A=beta[:-1, None], b=beta[-1:])
    return MF.Polynomial(degree, w=beta[:, None])


CASES = [("constant", [0.7], 0), ("linear", [-0.004, 0.9], 0), ("polynomial", [0.8, -6e-3, 3e-5], 2)]


def test_reference_against_central_differences():
    n = 60
    x, y = series(n)
    beta = np.array([0.8, -6e-3 * 251 / n, 3e-5 * (251 / n) ** 2])
    ok = O.OSquaredExponential(variance=0.6, lengthscales=7.0)
    lml, _, gm, _, Phi = ref_eval(x, y, ok, 0.05, "polynomial", beta, 2)

    def f(b):
        return O.OGPR(x, y - Phi @ b, ok, noise_variance=0.05).log_marginal_likelihood()

    assert abs(f(beta) - lml) <= 1e-12 * abs(lml)
    for k in range(3):
        # logML is quadratic in β: the central difference has no truncation error, so the step is
        # chosen for rounding alone (a change of order one in the residual's largest entry)
        h = 0.25 / np.abs(Phi[:, k]).max()
        e = np.zeros(3)
        e[k] = h
        fd = (f(beta + e) - f(beta - e)) / (2 * h)
        print(f"component {k}: Phi^T alpha {gm[k]:.12e}  central difference {fd:.12e}")
        assert abs(fd - gm[k]) <= 1e-7 * abs(gm[k]), (k, fd, gm[k])


# ------------------------------------------------------------------ structure -------------
def test_shapes_and_defaults():
    c, l, p = MF.Constant(), MF.Linear(), MF.Polynomial(2)
    assert c.c.shape == (1,) and c.c.value[0] == 0.0
    assert l.A.shape == (1, 1) and l.A.value[0, 0] == 1.0 and l.b.shape == (1,) and l.b.value[0] == 0.0
    assert p.w.shape == (3, 1) and not p.w.value.any()  # zeros: see the class docstring
    assert MF.Zero().parameters == () and isinstance(c, MF.MeanFunction)
    for mf in (c, l, p):
        assert all(q.trainable and q.transform_name == "Identity" for q in mf.parameters)
    assert [n for n, _ in l._param_paths()] == ["A", "b"]
    assert MF.Linear(A=np.ones((3, 1))).n_coef == 4
    with pytest.raises(NotImplementedError):
        MF.Polynomial(5)
    with pytest.raises(ValueError):
        MF.Polynomial(2, w=np.zeros(4))
    x = np.linspace(-2.0, 3.0, 7)[:, None]
    for kind, beta, deg in CASES:
        assert np.allclose(make_mean(kind, beta, deg)(x)[:, 0], mean_basis(kind, x, deg) @ np.asarray(beta), rtol=1e-15)


@pytest.mark.parametrize("kind,beta,deg", CASES)
def test_theta_row_and_variable_order_with_se(kind, beta, deg):
    x, y = series(20)
    mf = make_mean(kind, beta, deg)
    m = gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential(), mean_function=mf, noise_variance=0.1)
    assert m.mean_function is mf
    row = m.theta_row()
    nb = len(beta)
    assert row.shape == (N.GPX_THETA_STRIDE,)
    assert np.array_equal(row[:3], [1.0, 1.0, m.likelihood.variance.value])
    assert np.array_equal(row[3:3 + nb], beta) and np.all(row[3 + nb:] == 1.0)
    # tf.Module order: kernel.*, likelihood.variance, mean_function.* (attribute names sorted)
    names = [v.name for v in m.trainable_variables]
    assert names[:3] == ["lengthscales:0", "variance:0", "variance:0"]
    assert names[3:] == {"constant": ["c:0"], "linear": ["A:0", "b:0"], "polynomial": ["w:0"]}[kind]
    assert m.parameters[3:] == mf.parameters
    sp = m.mean_spec()
    assert (sp.kind, sp.n_coef) == ({"constant": 1, "linear": 2, "polynomial": 3}[kind], nb)
    cols, lower, tcode = m.theta_layout(m.trainable_variables, transforms=True)
    assert cols.tolist() == list(range(3 + nb)) and tcode.tolist() == [0, 0, 0] + [1] * nb
    assert lower.tolist() == [0.0, 0.0, 1e-6] + [0.0] * nb
    assert [a.tolist() for a in m.theta_layout(m.trainable_variables)] == [cols.tolist(), lower.tolist()]
    # the chain rule: softplus variables × sigmoid(u), identity variables × 1
    g = np.arange(1.0, 17.0)
    loss, gu = m.loss_and_grad_unconstrained(lml=2.5, grad_theta=g)
    assert loss == -2.5
    assert np.array_equal(gu[3:], -g[3:3 + nb])
    assert np.array_equal(gu[:3], [-g[i] * p.dtheta_du() for i, p in enumerate(m.parameters[:3])])
    # set_trainable on the whole mean function, and on one of its parameters
    gpx.set_trainable(m.mean_function, False)
    assert len(m.trainable_variables) == 3
    gpx.set_trainable(mf.parameters[-1], True)
    assert m.theta_layout(m.trainable_variables)[0].tolist()[3:] == list(range(3 + nb - mf.parameters[-1].value.size,
                                                                                3 + nb))


def test_widest_reference_row_and_overfull_row():
    x, y = series(20)
    k = K.Exponential() + K.Periodic(K.SquaredExponential()) + K.Linear()
    m = gpx.models.GPR(data=(x, y), kernel=k, mean_function=MF.Polynomial(2, w=[[0.5], [-0.25], [0.125]]))
    assert m.n_kernel_params == 6
    row = m.theta_row()
    assert np.array_equal(row[7:10], [0.5, -0.25, 0.125]) and np.all(row[10:] == 1.0)  # 10 columns
    assert m.theta_layout(m.trainable_variables)[0].tolist() == list(range(10))
    # 4 × 3 kernel parameters + noise + 3 coefficients = 16 fits; one more coefficient does not
    def wide():
        return K.RationalQuadratic() + K.RationalQuadratic() + K.Periodic(K.SquaredExponential()) + K.Periodic(
            K.SquaredExponential())
    gpx.models.GPR(data=(x, y), kernel=wide(), mean_function=MF.Polynomial(2))
    with pytest.raises(ValueError, match="do not fit"):
        gpx.models.GPR(data=(x, y), kernel=wide(), mean_function=MF.Polynomial(3))
    with pytest.raises(NotImplementedError):  # Polynomial: one input column
        gpx.models.GPR(data=(np.zeros((4, 2)), np.zeros(4)), kernel=K.SquaredExponential(), mean_function=MF.Polynomial(1))
    with pytest.raises(ValueError):  # Linear's default A serves D = 1 only
        gpx.models.GPR(data=(np.zeros((4, 2)), np.zeros(4)), kernel=K.SquaredExponential(), mean_function=MF.Linear())
    with pytest.raises(NotImplementedError):
        gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential(), mean_function=lambda X: 0 * X)


def test_zero_and_none_mean_are_todays_model():
    x, y = series(20)
    for mf in (None, MF.Zero()):
        m = gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential(), mean_function=mf)
        assert m.mean_spec() is None and len(m.parameters) == 3
        assert np.array_equal(m.theta_row(), [1.0] * 16)
        assert [n for n, _ in m._param_paths()] == ["GPR.kernel.lengthscales", "GPR.kernel.variance",
                                                    "GPR.likelihood.variance"]


def test_print_summary_lists_mean_rows(capsys):
    x, y = series(20)
    m = gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential(), mean_function=MF.Linear(A=[[2.0]], b=[-1.0]))
    rows = {r[0]: r for r in gpx.utilities.summary_rows(m)}
    assert list(rows)[-2:] == ["GPR.mean_function.A", "GPR.mean_function.b"]
    assert rows["GPR.mean_function.A"][2] == "Identity" and rows["GPR.mean_function.A"][4] == "(1, 1)"
    assert rows["GPR.mean_function.b"][2] == "Identity" and rows["GPR.mean_function.b"][3] is True
    gpx.print_summary(m)
    out = capsys.readouterr().out
    assert "GPR.mean_function.A" in out and "Identity" in out


def test_svgp_still_refuses_and_stream_refuses_before_the_device():
    with pytest.raises(NotImplementedError):
        gpx.models.SVGP(kernel=K.SquaredExponential(), likelihood=gpx.likelihoods.Gaussian(0.1),
                        inducing_variable=np.zeros((3, 1)), mean_function=MF.Constant())
    x, y = series(20)
    ms = [gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential()),
          gpx.models.GPR(data=(x, y), kernel=K.SquaredExponential(), mean_function=MF.Polynomial(2))]
    # (no engine is created: the refusal comes before any device call, so it is the same without a GPU)
    with pytest.raises(NotImplementedError, match="model 1.*Polynomial"):
        gpx.optimizers.Scipy().minimize_stream(ms, width=2)


# ------------------------------------------------------------------ host helpers ----------
def _ptr(a):
    return a.ctypes.data


def test_host_helpers_transform_codes():
    lib = N.load_library()  # (loads without a GPU, as tests/test_abi.py relies on)
    rng = np.random.default_rng(5)
    n_fits, P, B = 5, 6, 9
    U = np.ascontiguousarray(rng.normal(0.0, 3.0, (n_fits, P)))
    U[0, 0], U[1, 1], U[2, 4] = 0.0, -40.0, -3.5e-3
    rows = np.array([7, 0, 3, 8, 2], dtype=np.int32)
    cols = np.array([0, 1, 2, 3, 4, 5], dtype=np.int32)
    lower = np.array([0.0, 0.0, 1e-6, 0.0, 0.0, 0.0])
    tcode = np.array([0, 0, 0, 1, 1, 1], dtype=np.int32)
    th_old = np.ones((B, 16))
    th_new = np.ones((B, 16))
    z = np.zeros(P, dtype=np.int32)
    assert lib.gpx_host_theta_rows(n_fits, P, _ptr(U), _ptr(rows), _ptr(cols), _ptr(lower), _ptr(th_old)) == 0
    assert lib.gpx_host_theta_rows_t(n_fits, P, _ptr(U), _ptr(rows), _ptr(cols), _ptr(lower), _ptr(z), _ptr(th_new)) == 0
    assert np.array_equal(th_old, th_new)  # all-softplus codes: the old helper's bits
    assert lib.gpx_host_theta_rows_t(n_fits, P, _ptr(U), _ptr(rows), _ptr(cols), _ptr(lower), _ptr(tcode), _ptr(th_new)) == 0
    for k, b in enumerate(rows):
        for v in range(P):
            if tcode[v]:
                assert th_new[b, v] == U[k, v]
            else:  # parameter.py's arithmetic, bit for bit (and the old helper's)
                p = gpx.Parameter(1.0, lower=float(lower[v]))
                p.set_unconstrained(U[k, v])
                assert th_new[b, v] == p.value == th_old[b, v]
    untouched = np.setdiff1d(np.arange(B), rows)
    assert np.all(th_new[untouched] == 1.0) and np.all(th_new[:, P:] == 1.0)
    lml = rng.normal(0, 5, B)
    grad = rng.normal(0, 5, (B, 16))
    loss0, loss1 = np.empty(n_fits), np.empty(n_fits)
    g0, g1 = np.empty((n_fits, P)), np.empty((n_fits, P))
    assert lib.gpx_host_loss_grad_u(n_fits, P, _ptr(U), _ptr(rows), _ptr(cols), _ptr(lml), _ptr(grad), _ptr(loss0), _ptr(g0)) == 0
    assert lib.gpx_host_loss_grad_u_t(n_fits, P, _ptr(U), _ptr(rows), _ptr(cols), _ptr(z), _ptr(lml), _ptr(grad),
                                      _ptr(loss1), _ptr(g1)) == 0
    assert np.array_equal(loss0, loss1) and np.array_equal(g0, g1)
    assert lib.gpx_host_loss_grad_u_t(n_fits, P, _ptr(U), _ptr(rows), _ptr(cols), _ptr(tcode), _ptr(lml), _ptr(grad),
                                      _ptr(loss1), _ptr(g1)) == 0
    assert np.array_equal(loss1, -lml[rows])
    for k, b in enumerate(rows):
        for v in range(P):
            if tcode[v]:
                assert g1[k, v] == -grad[b, v]
            else:
                p = gpx.Parameter(1.0)
                p.set_unconstrained(U[k, v])
                assert g1[k, v] == -grad[b, v] * p.dtheta_du() == g0[k, v]
    bad = np.array([0, 0, 2, 0, 0, 0], dtype=np.int32)
    assert lib.gpx_host_theta_rows_t(n_fits, P, _ptr(U), _ptr(rows), _ptr(cols), _ptr(lower), _ptr(bad), _ptr(th_new)) == N.GPX_BAD_ARG
    assert ctypes.sizeof(N.GpxMeanSpec) == 16
