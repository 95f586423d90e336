"""Time the device sampler (engine.sample_mvn -> gpx_sample_mvn) beside the torch expression it
replaces, torch.linalg.cholesky(cov + jitter·I) @ whiteᵀ + mean, on the same device in the same
process: per shape (B, M, S) a warm-up, then the median HIP-event time of --reps calls of each,
alternating (profiles/samples.md). Prints one markdown table row per shape.

    python tools/sample_bench.py [--reps 30] [--warmup 5] [--shapes 20x150x1024,1x1024x64,8x30x16]
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from portfoliooptgp_amd import engine as E  # noqa: E402

JITTER = 1e-6


def problem(B, M, S, dev, seed=0):
    """SE posterior-like covariances (ℓ = 5 on a half-day grid plus a small nugget), random means / whites"""
    rng = np.random.default_rng(seed)
    x = np.linspace(0.0, M / 2.0, M)
    base = np.exp(-0.5 * (x[:, None] - x[None, :]) ** 2 / 25.0)
    cov = np.stack([(1.0 + 0.05 * b) * base + 1e-4 * np.eye(M) for b in range(B)])
    t = lambda a: torch.as_tensor(a, device=dev)  # noqa: E731
    return t(rng.standard_normal((B, M))), t(cov), t(rng.standard_normal((B, S, M)))


def torch_baseline(mean, cov, white):
    M = cov.shape[-1]
    L = torch.linalg.cholesky(cov + JITTER * torch.eye(M, dtype=cov.dtype, device=cov.device))
    return white @ L.transpose(-1, -2) + mean[:, None, :]


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--shapes", default="20x150x1024,1x1024x64,8x30x16")
    ap.add_argument("--device", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("sample_bench needs the GPU: no timing is taken without one")
    dev = f"cuda:{a.device}"
    print("| B | M | S | gpx_sample_mvn ms [min–max] | torch baseline ms [min–max] | gpx ÷ torch | max abs difference |")
    print("|---|---|---|---|---|---|---|")
    for shape in a.shapes.split(","):
        B, M, S = (int(v) for v in shape.split("x"))
        mean, cov, white = problem(B, M, S, dev)
        diff = float((E.sample_mvn(mean, cov, white, JITTER) - torch_baseline(mean, cov, white)).abs().max())
        # alternate the two so drift on a shared host hits both alike
        g, t = [], []
        for _ in range(3):
            g.append(timed(lambda: E.sample_mvn(mean, cov, white, JITTER), a.reps // 3, a.warmup))
            t.append(timed(lambda: torch_baseline(mean, cov, white), a.reps // 3, a.warmup))
        gm, tm = float(np.median([v[0] for v in g])), float(np.median([v[0] for v in t]))
        print(f"| {B} | {M} | {S} | {gm:.3f} [{min(v[1] for v in g):.3f}–{max(v[2] for v in g):.3f}] | "
              f"{tm:.3f} [{min(v[1] for v in t):.3f}–{max(v[2] for v in t):.3f}] | {gm / tm:.2f} | {diff:.2e} |", flush=True)


if __name__ == "__main__":
    main()
