"""The SGPR restatement (tests/sgpr_numpy.py) on the CPU: its hand-written gradients against
central finite differences of the GPflow-route bound, its two routes against each other, and the
bound against the exact log marginal likelihood it can never exceed."""
import numpy as np
import pytest

from oracle import gp_oracle as O
from tests.sgpr_numpy import NumpySGPR
from tests.test_oracle import oracle_kernel


def _case(fam, n=57, M=9, D=2, seed=0, noise=0.3):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, D))
    Y = np.sin(X[:, 0]) + 0.3 * np.cos(2 * X[:, -1]) + 0.1 * rng.standard_normal(n)
    Z = rng.uniform(0, 10, (M, D))
    k = oracle_kernel(fam)
    for p in k.params():
        p.value = float(np.exp(rng.uniform(-0.2, 0.8)))
    return NumpySGPR(k, X, Y, Z, noise_variance=noise)


def _fd(m, set_value, x0, h):
    set_value(x0 + h)
    fp = m.elbo("gpflow")
    set_value(x0 - h)
    fm = m.elbo("gpflow")
    set_value(x0)
    return (fp - fm) / (2 * h)


@pytest.mark.parametrize("fam", ["se", "exp+per+lin", "se*m12"])
@pytest.mark.parametrize("route", ["gpflow", "w"])
def test_gradients_match_central_differences(fam, route):
    m = _case(fam, seed=len(fam))
    F, g = m.elbo_and_grads(route)
    # the routes differ by rounding amplified by cond(Kmm) (≤ ~1e7 here: unit-scale kernels on a
    # 1e-6 jitter), so eps · cond ~ 1e-9 relative at the worst
    assert F == pytest.approx(m.elbo("gpflow"), rel=1e-8)
    scale = 1.0 + max(np.abs(g["theta"]).max(), abs(g["noise"]), np.abs(g["Z"]).max())
    for i, p in enumerate(m.kernel.params()):
        fd = _fd(m, lambda v, p=p: setattr(p, "value", v), p.value, 1e-6 * max(1.0, p.value))
        assert abs(fd - g["theta"][i]) <= 2e-6 * scale, (fam, p.name, fd, g["theta"][i])
    fd = _fd(m, lambda v: setattr(m.noise, "value", v), m.noise.value, 1e-6)
    assert abs(fd - g["noise"]) <= 2e-6 * scale, (fam, fd, g["noise"])
    Z0 = m.Z.copy()
    for (i, d) in [(0, 0), (3, 1), (8, 0), (5, 1)]:
        def setz(v, i=i, d=d):
            m.Z = Z0.copy()
            m.Z[i, d] = v
        fd = _fd(m, setz, Z0[i, d], 1e-6)
        assert abs(fd - g["Z"][i, d]) <= 2e-6 * scale, (fam, i, d, fd, g["Z"][i, d])


def test_unconstrained_gradient_matches_central_differences():
    m = _case("se", seed=4)
    u0 = m.get_u()
    loss, gu = m.loss_and_grad_u()
    assert len(gu) == len(u0) == m.Z.size + 3
    for k in (0, 7, len(u0) - 3, len(u0) - 2, len(u0) - 1):
        e = np.zeros_like(u0)
        e[k] = 1e-6
        m.set_u(u0 + e)
        fp = m.training_loss()
        m.set_u(u0 - e)
        fm = m.training_loss()
        assert abs((fp - fm) / 2e-6 - gu[k]) <= 2e-6 * (1 + np.abs(gu).max()), k
    m.set_u(u0)
    assert m.training_loss() == pytest.approx(loss, rel=1e-13)


def test_routes_agree_on_predictions():
    m = _case("se*m12", seed=6)
    xs = np.random.default_rng(7).uniform(-1, 11, (31, 2))
    (ma, va), (mb, vb) = m.predict_f(xs, "gpflow"), m.predict_f(xs, "w")
    np.testing.assert_allclose(ma, mb, rtol=1e-9, atol=1e-11)
    np.testing.assert_allclose(va, vb, rtol=1e-9, atol=1e-11)
    assert np.all(va > 0)
    np.testing.assert_allclose(m.predict_y(xs)[1] - va, m.noise.value, rtol=1e-12)


def test_bound_with_z_equal_x_is_just_below_exact_logml():
    """With Z = X the Titsias bound is tight up to the 1e-6 jitter on Kmm: F ≤ logML, and the gap
    is small (2.7e-4 measured at N = 57 when these formulas were first checked)."""
    m = _case("se", n=57, M=9, D=2, seed=2, noise=0.3)
    m.Z = m.X.copy()
    exact = O.OGPR(m.X, m.Y, m.kernel, noise_variance=0.3).log_marginal_likelihood()
    for route in ("gpflow", "w"):
        F = m.elbo(route)
        assert F <= exact + 1e-9 * abs(exact)
        assert exact - F <= 5e-3, (route, exact - F)
