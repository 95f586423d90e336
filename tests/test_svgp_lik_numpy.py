"""Pin the restatement of SVGP's per-point ELBO (tests/svgp_lik_numpy.py) on the CPU: its two routes
against each other, every gradient block against central differences of the ELBO itself, the
Gaussian likelihood against the SVGP oracle's closed form, Z = X against the VGP restatement, and
the device parity cases (tests/svgp_lik_cases.py) against the caps on their bars."""
import numpy as np
import pytest

from oracle import svgp_oracle as S
from tests import svgp_lik_cases as C
from tests.svgp_lik_numpy import BLOCKS, NumpySVGPLik
from tests.test_oracle import oracle_kernel
from tests.vgp_numpy import NumpyVGP


def _problem(n=40, M=7, D=1, seed=0, fam="se", likelihood="studentt", num_data=None):
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, D))
    Y = np.sin(X[:, :1]) + 0.1 * rng.standard_normal((n, 1))
    Y[rng.choice(n, 3, replace=False), 0] += 2.0
    Z = rng.uniform(0, 10, (M, D))
    R = np.tril(rng.standard_normal((M, M)) * 0.2)
    R[np.diag_indices(M)] = rng.uniform(0.4, 1.2, M)
    m = NumpySVGPLik(oracle_kernel(fam), Z, likelihood=likelihood, scale=0.3, variance=0.05, df=3.0,
                     num_data=n if num_data is None else num_data, q_mu=rng.standard_normal(M) * 0.3, q_sqrt=R)
    return m, X, Y


@pytest.mark.parametrize("likelihood", ["studentt", "gaussian"])
@pytest.mark.parametrize("fam,D", [("se", 1), ("m32", 2), ("exp+per+lin", 1), ("se*m12", 2)])
def test_the_two_routes_agree(fam, D, likelihood):
    """N = 40, M = 7 from uniform draws: cond(Kmm) stays below 1e5, where two fp64 routes agree to
    far better than 1e-10 (F) and 1e-8 (gradient blocks)."""
    m, X, Y = _problem(D=D, seed=1, fam=fam, likelihood=likelihood, num_data=400)
    assert np.linalg.cond(m.kmm()) < 1e5
    aux = {}
    Fa, ga = m.elbo_and_grads(X, Y, "gpflow", aux=aux)
    Fb, gb = m.elbo_and_grads(X, Y, "w")
    assert abs(Fa - Fb) <= 1e-10 * abs(Fa)
    for k in BLOCKS:
        a, b = np.asarray(ga[k]), np.asarray(gb[k])
        assert np.abs(a - b).max() <= 1e-8 * (1.0 + np.abs(a).max()), k
    if likelihood == "studentt":   # the outliers' rows push g_v above zero
        assert (aux["g_v"] > 0).any() and (aux["g_v"] < 0).any()
    for fn in ("predict_f", "predict_y"):
        xs = np.random.default_rng(2).uniform(-1, 11, (9, D))
        for a, b in zip(getattr(m, fn)(xs, "gpflow"), getattr(m, fn)(xs, "w")):
            assert np.abs(a - b).max() <= 1e-9 * (1.0 + np.abs(a).max())


@pytest.mark.parametrize("route", ["gpflow", "w"])
@pytest.mark.parametrize("fam,likelihood", [("se", "studentt"), ("m12", "studentt"), ("rq", "studentt"),
                                            ("exp+per+lin", "studentt"), ("se*m12", "studentt"),
                                            ("m52", "gaussian")])
def test_gradients_match_central_differences(fam, likelihood, route):
    """Every block (Z, θ, the likelihood parameter, q_mu, q_sqrt) in unconstrained space, N = 40, M = 7."""
    m, X, Y = _problem(seed=3, fam=fam, likelihood=likelihood, num_data=100)
    elbo, g = m.elbo_and_grads(X, Y, route)
    # the unconstrained chain of oracle/svgp_oracle.py's loss_and_grad_u, for this route's blocks
    parts = [-g["Z"].ravel(),
             np.array([-g["theta"][i] * p.dtheta_du() for i, p in enumerate(m.kernel.params())]
                      + [-g["lik"] * m.noise.dtheta_du()]),
             -g["q_mu"].ravel(), -S.fill_triangular_inverse(g["q_sqrt"])]
    grad = np.concatenate(parts)
    u0 = m.get_u()
    assert grad.shape == u0.shape
    h = 1e-6
    fd = np.empty_like(u0)
    for i in range(u0.size):
        up, um = u0.copy(), u0.copy()
        up[i] += h
        um[i] -= h
        m.set_u(up)
        lp = m.training_loss(X, Y, route)
        m.set_u(um)
        lm = m.training_loss(X, Y, route)
        fd[i] = (lp - lm) / (2 * h)
    m.set_u(u0)
    assert m.training_loss(X, Y, route) == pytest.approx(-elbo, rel=1e-14)
    np.testing.assert_allclose(grad, fd, rtol=2e-5, atol=2e-5 * (1 + np.abs(fd).max()))
    if route == "gpflow":   # the inherited flattening is this one (set_u(get_u()) moves θ by an ulp)
        loss, gu = m.loss_and_grad_u(X, Y)
        assert loss == pytest.approx(-elbo, rel=1e-13)
        np.testing.assert_allclose(gu, grad, rtol=1e-10, atol=1e-10 * (1 + np.abs(grad).max()))


@pytest.mark.parametrize("fam,D", [("se", 1), ("exp+per+lin", 1), ("m32", 2)])
def test_gaussian_likelihood_equals_the_svgp_oracle(fam, D):
    m, X, Y = _problem(D=D, seed=4, fam=fam, likelihood="gaussian", num_data=250)
    om = S.OSVGP(oracle_kernel(fam), m.Z, num_data=250, noise_variance=0.05, q_mu=m.q_mu, q_sqrt=m.q_sqrt)
    Fo, go = om.elbo_and_grads(X, Y)
    for route in ("gpflow", "w"):
        F, g = m.elbo_and_grads(X, Y, route)
        assert abs(F - Fo) <= 1e-10 * abs(Fo), route
        for k, ko in (("theta", "theta"), ("lik", "noise"), ("Z", "Z"), ("q_mu", "q_mu"), ("q_sqrt", "q_sqrt")):
            a, b = np.asarray(g[k]), np.asarray(go[ko])
            assert np.abs(a - b).max() <= 1e-10 * (1.0 + np.abs(b).max()), (route, k)
    xs = np.random.default_rng(5).uniform(-1, 11, (11, D))
    for a, b in zip(m.predict_y(xs), om.predict_y(xs)):
        assert np.abs(a - b).max() <= 1e-10 * (1.0 + np.abs(b).max())


@pytest.mark.parametrize("likelihood", ["studentt", "gaussian"])
def test_z_equal_x_is_vgp(likelihood, monkeypatch):
    """Whitened SVGP with Z = X is VGP, M = N = 30 — as an identity of the algebra, so with the
    jitter of both restatements set to zero. With GPflow's 1e-6 the two models differ, and not by
    rounding: VGP's marginal mean is L q with L Lᵀ = K + 1e-6 I, SVGP's is Kᵀ L⁻ᵀ q = L q − 1e-6 L⁻ᵀ q,
    because the jitter enters Kmm and never the cross-covariance Kmn (with an SE kernel on these
    inputs the two ELBOs then differ by 1.2e-5 relative, 1e-3 absolute). Matern-3/2 at unit lengthscale keeps cond(K) near 1e3 without jitter."""
    import tests.svgp_lik_numpy as SL
    import tests.vgp_numpy as VN
    monkeypatch.setattr(SL, "JITTER", 0.0)
    monkeypatch.setattr(VN, "JITTER", 0.0)
    n = 30
    rng = np.random.default_rng(6)
    X = (np.linspace(0, 10, n) + rng.uniform(-0.1, 0.1, n))[:, None]
    Y = np.sin(X) + 0.1 * rng.standard_normal((n, 1))
    Y[[4, 17], 0] -= 2.0
    q = 0.5 * rng.standard_normal(n)
    R = np.tril(0.1 * rng.standard_normal((n, n)), -1) + np.diag(rng.uniform(0.3, 1.5, n))
    sv = NumpySVGPLik(oracle_kernel("m32"), X, likelihood=likelihood, scale=0.3, variance=0.05, df=3.0,
                      num_data=n, q_mu=q, q_sqrt=R)
    vg = NumpyVGP(oracle_kernel("m32"), X, Y, likelihood=likelihood, scale=0.3, variance=0.05, df=3.0)
    vg.q, vg.R = q, R
    assert np.linalg.cond(sv.kmm()) < 1e5
    np.testing.assert_array_equal(sv.kmm(), vg.kxx())
    Fv, gv = vg.elbo_and_grads()
    for route in ("gpflow", "w"):
        F, g = sv.elbo_and_grads(X, Y, route)
        assert abs(F - Fv) <= 1e-10 * abs(Fv), route
        # q_mu and q_sqrt are the same variables in both models. VGP's θ gradient moves the one
        # matrix K; here K appears as Kmm, Kmn and k_nn, and "theta" sums all three: equal too
        for k in ("theta", "lik", "q_mu", "q_sqrt"):
            a, b = np.asarray(g[k]), np.asarray(gv[k])
            assert np.abs(a - b).max() <= 1e-10 * (1.0 + np.abs(b).max()), (route, k)
    xs = rng.uniform(-1, 11, (8, 1))
    for a, b in zip(sv.predict_y(xs), vg.predict_y(xs)):
        assert np.abs(a - b).max() <= 1e-10 * (1.0 + np.abs(b).max())


@pytest.mark.parametrize("name", list(C.CASES))
def test_device_parity_cases_stay_inside_the_caps(name):
    """What tests/test_svgp_lik_gpu.py asserts before it compares the device, here without one; and
    that the outlier cases make g_v take both signs."""
    ref = C.reference(name)
    print(f"{name}: cond={ref['cond']:.3g} tolF/|F|={ref['tolF'] / abs(ref['F']):.3g} "
          + " ".join(f"{k}={ref['tolg'][k] / (1 + np.abs(ref['g'][k]).max()):.3g}" for k in BLOCKS)
          + f" g_v>0: {np.mean(ref['g_v'] > 0):.3f}")
    C.assert_inside_caps(name, ref)
    if C.CASES[name][5]:
        assert (ref["g_v"] > 0).any() and (ref["g_v"] < 0).any()
