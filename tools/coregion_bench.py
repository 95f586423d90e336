"""Coregion against the two-term product it replaces: one loss+gradient evaluation and one
predict_f(full_cov=True) at the P rows of one day, for Exp(dims 0..3) x Coregion(5, 1) on 5 stacked
assets of 67 and 820 rows (the issue's shapes: Np = 384 and 4160, no multiples of 128, so the
contraction runs 64-tiles) and of 128 and 819 rows (Np = 640 and 4096: the 128-tile instances),
beside the two-term Exp(dims 0..3) x Exp(index column) spec (the EPI_CONTRACT2 path, config C4's
kernel) on the same data — all in one process on one device. Per
configuration: the median of `reps` calls after `warmup`, each timed with HIP events on the call's
stream (the call synchronises before it returns, so the interval is the whole call: upload,
kernels, download), then one profiled evaluation for the library's own phase split. Prints one JSON
line per configuration and the Coregion / Exp x Exp ratios; profiles/coregion.md records a run."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from portfoliooptgp_amd import kernels as K  # noqa: E402
from portfoliooptgp_amd import trainer  # noqa: E402
from portfoliooptgp_amd.engine import Engine  # noqa: E402
from portfoliooptgp_amd.kernels import compile_spec  # noqa: E402

P, DF = 5, 4


def stacked(n_per):
    """5 assets of n_per rows: 4 z-scored random-walk features, returns that co-move; stacked"""
    rng = np.random.default_rng(11)
    common = rng.standard_normal(n_per)
    series = []
    for p in range(P):
        F = np.cumsum(rng.standard_normal((n_per, DF)), axis=0)
        F = (F - F.mean(0)) / F.std(0, ddof=1)
        y = (0.7 if p % 2 == 0 else -0.5) * common + 0.3 * np.tanh(F[:, 0]) + 0.1 * rng.standard_normal(n_per)
        series.append((F, y[:, None]))
    return trainer.stack_assets(series)


def configs(idx):
    def row(vals):
        th = np.ones(16)
        th[:len(vals)] = vals
        return th
    cg = K.Exponential(active_dims=slice(0, idx)) * K.Coregion(output_dim=P, rank=1, active_dims=[idx])
    W = [0.6, -0.4, 0.5, -0.3, 0.7]
    return {
        "expxexp": (K.Exponential(active_dims=slice(0, idx)) * K.Exponential(active_dims=slice(idx, idx + 1)),
                    row([2.0, 1.0, 2.0, 1.0, 1e-3])),
        "expxcoreg": (cg, row([2.0, 1.0] + W + [0.5] * P + [1e-3])),
    }


def timed(fn, reps, warmup):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return dict(median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms))


def time_config(name, kernel, row, X, Y, idx, reps, warmup):
    eng = Engine([X], [Y], [compile_spec(kernel, X.shape[1])])
    theta = row[None, :].copy()
    lml, _, info = eng.lml_grad([0], theta)
    assert not info.any(), info
    ev = timed(lambda: eng.lml_grad([0], theta), reps, warmup)
    day = np.concatenate([np.tile(X[-1, :idx], (P, 1)), np.arange(P, dtype=np.float64)[:, None]], axis=1)
    pr = timed(lambda: eng.predict([0], theta, [day], False, full_cov=True), reps, warmup)
    eng.ctx.set_profiling(True)
    eng.lml_grad([0], theta)
    tm = eng.last_timing()
    eng.ctx.set_profiling(False)
    Np = (int(X.shape[0]) + 63) // 64 * 64
    tile = 128 if Np % 128 == 0 and Np >= 512 else 64   # (gemm_tile's rule for the contraction)
    out = dict(config=name, N=int(X.shape[0]), Np=Np, contract_tile=tile, eval=ev, predict_full_cov=pr, reps=reps, factor_ms=tm.factor_ms,
               solve_ms=tm.alpha_ms, contract_reduce_ms=tm.grad_ms, lml=float(lml[0]))
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n-per", type=int, nargs="+", default=[67, 128, 819, 820])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for n_per in args.n_per:
        X, Y, idx = stacked(n_per)
        res = {}
        for name, (kernel, row) in configs(idx).items():
            res[name] = time_config(name, kernel, row, X, Y, idx, args.reps, args.warmup)
            print(json.dumps(res[name]), flush=True)
        a, b = res["expxcoreg"], res["expxexp"]
        print(json.dumps(dict(N=int(X.shape[0]), pair="expxcoreg/expxexp",
                              ratio_eval=a["eval"]["median_ms"] / b["eval"]["median_ms"],
                              ratio_predict=a["predict_full_cov"]["median_ms"] / b["predict_full_cov"]["median_ms"],
                              ratio_contract=a["contract_reduce_ms"] / max(b["contract_reduce_ms"], 1e-9),
                              ratio_factor=a["factor_ms"] / max(b["factor_ms"], 1e-9))), flush=True)


if __name__ == "__main__":
    main()
