"""The VGP restatement (tests/vgp_numpy.py) on the CPU: its hand-written gradients against central
finite differences of the GPflow-route ELBO, the 20-point Gauss–Hermite rule against the Gaussian
closed form, the ELBO at the optimal q against the exact log marginal likelihood, and the moments
of q(f) at the initial q."""
import math

import numpy as np
import pytest

from oracle.gp_oracle import LOG2PI
from tests.test_oracle import oracle_kernel
from tests.vgp_numpy import JITTER, NumpyVGP, gauss_hermite


def _case(lik, fam="se+m12", n=12, D=2, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 4, (n, D))
    Y = np.sin(X[:, 0]) + 0.3 * np.cos(2 * X[:, -1]) + 0.1 * rng.standard_normal(n)
    Y[::5] += 2.5  # outliers
    k = oracle_kernel(fam)
    for p in k.params():
        p.value = float(np.exp(rng.uniform(-0.2, 0.8)))
    m = NumpyVGP(k, X, Y, likelihood=lik, scale=0.4, variance=0.3, df=3.0)
    m.q = 0.5 * rng.standard_normal(n)
    m.R = np.tril(0.2 * rng.standard_normal((n, n)), -1) + np.diag(rng.uniform(0.3, 1.5, n))
    return m


def _fd(m, set_value, x0, h):
    set_value(x0 + h)
    fp = m.elbo("gpflow")
    set_value(x0 - h)
    fm = m.elbo("gpflow")
    set_value(x0)
    return (fp - fm) / (2 * h)


@pytest.mark.parametrize("lik", ["gaussian", "studentt"])
def test_gradients_match_central_differences(lik):
    """Every block of the "gpflow" route: N = 12, D = 2, a two-term kernel, random q and
    lower-triangular R with a positive diagonal. Central differences of step h carry an h² f‴
    truncation error and an eps |F| / h rounding error: ~1e-9 + 1e-9 at h = 1e-6 on |F| ~ 30, so
    2e-6 · (1 + max|g|) leaves three decades."""
    m = _case(lik)
    F, g = m.elbo_and_grads("gpflow")
    assert F == pytest.approx(m.elbo("gpflow"), rel=1e-13)
    scale = 1.0 + max(np.abs(g["theta"]).max(), abs(g["lik"]), np.abs(g["q_mu"]).max(), np.abs(g["q_sqrt"]).max())
    assert len(g["theta"]) == len(m.kernel.params()) == 4
    for i, p in enumerate(m.kernel.params()):
        fd = _fd(m, lambda v, p=p: setattr(p, "value", v), p.value, 1e-6 * max(1.0, p.value))
        assert abs(fd - g["theta"][i]) <= 2e-6 * scale, (lik, p.name, fd, g["theta"][i])
    fd = _fd(m, lambda v: setattr(m.lik, "value", v), m.lik.value, 1e-6)
    assert abs(fd - g["lik"]) <= 2e-6 * scale, (lik, fd, g["lik"])
    q0 = m.q.copy()
    for i in range(len(q0)):
        def setq(v, i=i):
            m.q = q0.copy()
            m.q[i] = v
        fd = _fd(m, setq, q0[i], 1e-6)
        assert abs(fd - g["q_mu"][i]) <= 2e-6 * scale, (lik, i, fd, g["q_mu"][i])
    R0 = m.R.copy()
    assert np.all(np.triu(g["q_sqrt"], 1) == 0.0)
    for i in range(len(q0)):
        for j in range(i + 1):
            def setr(v, i=i, j=j):
                m.R = R0.copy()
                m.R[i, j] = v
            fd = _fd(m, setr, R0[i, j], 1e-6)
            assert abs(fd - g["q_sqrt"][i, j]) <= 2e-6 * scale, (lik, i, j, fd, g["q_sqrt"][i, j])


@pytest.mark.parametrize("lik", ["gaussian", "studentt"])
def test_w_route_matches_gpflow_route(lik):
    m = _case(lik, seed=3)
    Fa, ga = m.elbo_and_grads("gpflow")
    Fb, gb = m.elbo_and_grads("w")
    assert Fb == pytest.approx(Fa, rel=1e-9)
    for k in ("theta", "q_mu", "q_sqrt"):
        np.testing.assert_allclose(gb[k], ga[k], rtol=0, atol=1e-8 * (1 + np.abs(ga[k]).max()))
    assert gb["lik"] == pytest.approx(ga["lik"], rel=1e-8, abs=1e-8)


def test_gauss_hermite_rule_reproduces_gaussian_closed_form():
    """The generic 20-point rule applied to the Gaussian log-density: a quadratic is integrated
    exactly, so agreement to 1e-13 · (1 + |value|) pins nodes, weights and the 1/√π."""
    m = _case("gaussian", seed=5)
    rng = np.random.default_rng(6)
    mu, v = rng.standard_normal(12) * 2.0, rng.uniform(0.01, 5.0, 12)
    closed = m.variational_expectations(mu, v)[0]
    quad = gauss_hermite(lambda f: m.logp(f, m.Y[:, None]), mu, v)
    assert np.all(np.abs(quad - closed) <= 1e-13 * (1.0 + np.abs(closed))), np.abs(quad - closed).max()


def test_elbo_at_optimal_q_is_exact_log_marginal_likelihood():
    """Gaussian likelihood, q = Lᵀ(K̃+sI)⁻¹y and RRᵀ = I − Lᵀ(K̃+sI)⁻¹L: q(f) is the exact posterior,
    so the ELBO equals log N(y | 0, K̃ + sI). Bar 1e-8 · (1 + |F|) on a case with cond(K̃) <= 1e4:
    four decades above eps · cond."""
    m = _case("gaussian", fam="se", n=12, D=2, seed=7)
    for p in m.kernel.params():
        p.value = 0.6 if "length" in p.name else 1.3
    s, n = m.lik.value, len(m.Y)
    Kt = m.kxx()
    assert np.linalg.cond(Kt) <= 1e4, np.linalg.cond(Kt)
    L = np.linalg.cholesky(Kt)
    Ky = Kt + s * np.eye(n)
    m.q = L.T @ np.linalg.solve(Ky, m.Y)
    m.R = np.linalg.cholesky(np.eye(n) - L.T @ np.linalg.solve(Ky, L))
    Ly = np.linalg.cholesky(Ky)
    a = np.linalg.solve(Ly, m.Y)
    exact = -0.5 * n * LOG2PI - float(np.sum(np.log(np.diag(Ly)))) - 0.5 * float(a @ a)
    for route in ("gpflow", "w"):
        F = m.elbo(route)
        assert abs(F - exact) <= 1e-8 * (1.0 + abs(exact)), (route, F, exact)
    # and it is a maximum in q: the variational gradients vanish there
    _, g = m.elbo_and_grads("gpflow")
    assert np.abs(g["q_mu"]).max() <= 1e-8 * (1 + np.abs(m.q).max() / s)
    assert np.abs(g["q_sqrt"]).max() <= 1e-6


@pytest.mark.parametrize("route", ["gpflow", "w"])
def test_initial_q_gives_prior_moments(route):
    """At q = 0, R = I: μ = 0 and v = diag(K̃)."""
    m = _case("studentt", seed=8)
    m.q = np.zeros(12)
    m.R = np.eye(12)
    mu, v = m.moments(route)
    assert np.all(mu == 0.0)
    np.testing.assert_allclose(v, m.kernel.K_diag(m.X) + JITTER, rtol=1e-12)
    assert m.kl() == 0.0


def test_predict_y_quadrature_reduces_to_added_variance():
    m = _case("studentt", seed=9)
    xs = np.random.default_rng(1).uniform(0, 4, (7, 2))
    mf, vf = m.predict_f(xs)
    my, vy = m.predict_y(xs)
    np.testing.assert_allclose(my, mf, rtol=1e-12, atol=1e-14)
    np.testing.assert_allclose(vy, vf + m.lik.value ** 2 * 3.0, rtol=1e-11)
    assert np.all(vf > 0)
    assert math.isclose(m.df, 3.0)
