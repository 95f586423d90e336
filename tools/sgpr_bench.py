"""Time one SGPR bound+gradient evaluation (gpx_sgpr_elbo_grad) on one GPU, beside one SVGP
ELBO+gradient evaluation (gpx_svgp_elbo_grad) at the same shape in the same process, the two
alternated window by window so that both see the same machine state. Defaults: the C5 shape
(N=65536, M=1024, D=1, SE); the reference's SGPR cell is --n 113 --m 10 --span 10.
Usage: python tools/sgpr_bench.py [--n N] [--m M] [--reps R] [--windows W] [--cpu]"""
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
from portfoliooptgp_amd.engine import SGPREngine, SVGPEngine  # noqa: E402
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
    ap.add_argument("--n", type=int, default=65536)
    ap.add_argument("--m", type=int, default=1024)
    ap.add_argument("--span", type=float, default=360.0, help="inputs and the inducing grid cover [0, span]")
    ap.add_argument("--ell", type=float, default=2.0)
    ap.add_argument("--noise", type=float, default=1e-2)
    ap.add_argument("--reps", type=int, default=5, help="calls per timing window")
    ap.add_argument("--windows", type=int, default=5, help="alternating windows per model")
    ap.add_argument("--cpu", action="store_true",
                    help="also time one bound+gradient evaluation of the numpy restatement (tests/sgpr_numpy.py)")
    a = ap.parse_args()
    n, M = a.n, a.m
    rng = np.random.default_rng(0)
    X = np.sort(rng.uniform(0, a.span, (n, 1)), axis=0)
    Y = np.sin(X / (a.span / 18.0)) + 0.1 * rng.standard_normal((n, 1))
    Z = np.linspace(0, a.span, M)[:, None]
    k = gpx.kernels.SquaredExponential(lengthscales=a.ell, variance=1.0)
    spec = compile_spec(k, 1)
    theta = np.ones(16)
    theta[:3] = [a.ell, 1.0, a.noise]
    sg = SGPREngine(X, Y, spec, M)
    sv = SVGPEngine(X, Y, spec, M, num_data=n)
    q = rng.standard_normal(M) * 0.3
    R = np.tril(rng.standard_normal((M, M)) * 1e-3)
    R[np.diag_indices(M)] = rng.uniform(0.05, 0.2, M)
    f_sg = lambda: sg.elbo_grad(theta, Z)          # noqa: E731
    f_sv = lambda: sv.elbo_grad(theta, Z, q, R)    # noqa: E731
    for f in (f_sg, f_sv, f_sg, f_sv):             # warm both shapes up
        f()
    t_sg, t_sv = [], []
    for _ in range(a.windows):
        t_sg.append(window(f_sg, a.reps))
        t_sv.append(window(f_sv, a.reps))
    xs = np.linspace(0, a.span, 4096)[:, None]
    sg.predict(theta, Z, xs, False)
    t_pr = [window(lambda: sg.predict(theta, Z, xs, False), a.reps) for _ in range(a.windows)]
    Mp = (M + 63) // 64 * 64
    big = 3.0 * Mp * Mp * n            # G (SYRK, lower: M²N) + Y = (WᵀHW)·Kmn (2M²N)
    ms = lambda t: {"median": statistics.median(t) * 1e3, "min": min(t) * 1e3, "max": max(t) * 1e3}  # noqa: E731
    out = {"N": n, "M": M, "reps": a.reps, "windows": a.windows, "sgpr_eval_ms": ms(t_sg), "svgp_eval_ms": ms(t_sv),
           "sgpr_over_svgp": statistics.median(t_sg) / statistics.median(t_sv),
           "sgpr_big_gemm_tflops": big / statistics.median(t_sg) / 1e12, "sgpr_predict_ms_4096": ms(t_pr)}
    if a.cpu:  # host baseline: the restatement (test infrastructure) on the same inputs, one evaluation
        from oracle import gp_oracle as O
        from tests.sgpr_numpy import NumpySGPR
        om = NumpySGPR(O.OSquaredExponential(lengthscales=a.ell, variance=1.0), X, Y, Z, noise_variance=a.noise)
        # (its gradients go through a dense ∂K over [Z; X]: beyond a few thousand rows only the bound)
        grads = n + M <= 8192
        f_cpu = (lambda: om.elbo_and_grads("w")[0]) if grads else (lambda: om.elbo("w"))
        f_cpu()
        t2 = time.perf_counter()
        F_cpu = f_cpu()
        out["cpu_eval_ms"] = (time.perf_counter() - t2) * 1e3
        out["cpu_what"] = "bound+gradients" if grads else "bound only"
        out["cpu_threads"] = int(os.environ.get("OPENBLAS_NUM_THREADS") or os.environ.get("OMP_NUM_THREADS")
                                 or os.cpu_count())
        out["elbo_rel_diff"] = abs(sg.elbo_grad(theta, Z)[0] - F_cpu) / abs(F_cpu)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
