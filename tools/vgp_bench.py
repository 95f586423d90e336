"""Time one VGP ELBO+gradient evaluation (gpx_vgp_elbo_grad) on one GPU, beside one SVGP
ELBO+gradient evaluation (gpx_svgp_elbo_grad) with M = N inducing points at Z = X on the same data
in the same process, the two alternated window by window so that both see the same machine state.
Defaults: the reference's VGP cell (N = 113, SE kernel, StudentT likelihood, day offsets 0..360).
Usage: python tools/vgp_bench.py [--n N] [--likelihood studentt|gaussian] [--reps R] [--windows W] [--cpu]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import portfoliooptgp_amd as gpx  # noqa: E402
from portfoliooptgp_amd import _native as N  # noqa: E402
from portfoliooptgp_amd.engine import SVGPEngine, VGPEngine  # noqa: E402
from portfoliooptgp_amd.kernels import compile_spec  # noqa: E402


def window(fn, reps):
    """Seconds per call over one window of `reps` calls (each call ends in a stream synchronise)."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=113)
    ap.add_argument("--span", type=float, default=360.0, help="inputs cover [0, span] on a jittered grid")
    ap.add_argument("--ell", type=float, default=1.0)
    ap.add_argument("--likelihood", choices=("studentt", "gaussian"), default="studentt")
    ap.add_argument("--phi", type=float, default=1.0, help="StudentT scale / Gaussian variance")
    ap.add_argument("--df", type=float, default=3.0)
    ap.add_argument("--reps", type=int, default=50, help="calls per timing window")
    ap.add_argument("--windows", type=int, default=7, help="alternating windows per model")
    ap.add_argument("--cpu", action="store_true",
                    help="also time one ELBO+gradient evaluation of the numpy restatement (tests/vgp_numpy.py)")
    a = ap.parse_args()
    n = a.n
    rng = np.random.default_rng(0)
    X = (np.linspace(0, a.span, n) + rng.uniform(-0.3, 0.3, n) * a.span / n)[:, None]
    Y = np.sin(X / (a.span / 18.0)) + 0.1 * rng.standard_normal((n, 1))
    Y[rng.choice(n, max(1, n // 25), replace=False), 0] += 0.5
    k = gpx.kernels.SquaredExponential(lengthscales=a.ell, variance=1.0)
    spec = compile_spec(k, 1)
    theta = np.ones(16)
    theta[:3] = [a.ell, 1.0, a.phi]
    st = a.likelihood == "studentt"
    vg = VGPEngine(X, Y, spec, N.GPX_LIK_STUDENT_T if st else N.GPX_LIK_GAUSSIAN, df=a.df)
    sv = SVGPEngine(X, Y, spec, n, num_data=n)
    q = rng.standard_normal(n) * 0.3
    R = np.tril(rng.standard_normal((n, n)) * 1e-3)
    R[np.diag_indices(n)] = rng.uniform(0.3, 1.5, n)
    th_sv = theta.copy()
    th_sv[2] = a.phi if not st else a.phi ** 2   # the SVGP path is Gaussian only: a noise variance
    f_vg = lambda: vg.elbo_grad(theta, q, R)          # noqa: E731
    f_sv = lambda: sv.elbo_grad(th_sv, X, q, R)       # noqa: E731
    for f in (f_vg, f_sv, f_vg, f_sv):                # warm both up
        f()
    t_vg, t_sv = [], []
    for _ in range(a.windows):
        t_vg.append(window(f_vg, a.reps))
        t_sv.append(window(f_sv, a.reps))
    xs = np.linspace(0, a.span, 1024)[:, None]
    vg.predict(theta, q, R, xs, True)
    t_pr = [window(lambda: vg.predict(theta, q, R, xs, True), a.reps) for _ in range(a.windows)]
    ms = lambda t: {"median": statistics.median(t) * 1e3, "min": min(t) * 1e3, "max": max(t) * 1e3}  # noqa: E731
    out = {"N": n, "likelihood": a.likelihood, "reps": a.reps, "windows": a.windows, "vgp_eval_ms": ms(t_vg),
           "svgp_m_eq_n_eval_ms": ms(t_sv), "vgp_over_svgp": statistics.median(t_vg) / statistics.median(t_sv),
           "vgp_predict_y_ms_1024": ms(t_pr)}
    if a.cpu:  # host baseline: the restatement (test infrastructure) on the same inputs, one evaluation
        from oracle import gp_oracle as O
        from tests.vgp_numpy import NumpyVGP
        om = NumpyVGP(O.OSquaredExponential(lengthscales=a.ell, variance=1.0), X, Y, likelihood=a.likelihood,
                      scale=a.phi, variance=a.phi, df=a.df)
        om.q, om.R = q, R
        om.elbo_and_grads("w")
        t2 = time.perf_counter()
        F_cpu = om.elbo_and_grads("w")[0]
        out["cpu_eval_ms"] = (time.perf_counter() - t2) * 1e3
        out["cpu_threads"] = int(os.environ.get("OPENBLAS_NUM_THREADS") or os.environ.get("OMP_NUM_THREADS")
                                 or os.cpu_count())
        out["elbo_rel_diff"] = abs(vg.elbo_grad(theta, q, R)[0] - F_cpu) / abs(F_cpu)
        out["cond_K"] = float(np.linalg.cond(om.kxx()))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
