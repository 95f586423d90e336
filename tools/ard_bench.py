"""ARD against isotropic: one loss+gradient evaluation at the C4 shape (N = 4096, D = 5: 4
z-scored random-walk features + z-scored time, as tools/prof_eval.py builds them), B = 1 and 32,
for Matern52 / Matern52-ARD and Exp x Exp / Exp(ARD, 4 dims) x Exp — all in one process on one
device. Per configuration: the median of `reps` evaluations after `warmup`, each timed with HIP
events on the call's stream (the call synchronises before it returns, so the interval is the whole
evaluation: upload, kernels, download), then one profiled evaluation for the library's own phase
split (factor / solves / contraction + reduce). Prints one JSON line per configuration and the
ARD / isotropic ratios; profiles/ard.md records a run."""
import argparse
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from portfoliooptgp_amd import kernels as K  # noqa: E402
from portfoliooptgp_amd.engine import Engine  # noqa: E402
from portfoliooptgp_amd.kernels import compile_spec  # noqa: E402
from bench import synthetic_series  # noqa: E402

D = 5


def c4_data(n, b):
    out = []
    for s in range(b):
        rng = np.random.default_rng(100 + s)
        feats = np.cumsum(rng.standard_normal((n, D - 1)), axis=0)
        X = np.hstack([feats, np.linspace(0.0, 1.0, n)[:, None]])
        X = (X - X.mean(0)) / X.std(0, ddof=1)
        out.append((X, synthetic_series(n, s)[1]))
    return out


def configs():
    """name -> (kernel, θ row): the ARD rows hold the isotropic ℓ in every ℓ_d slot."""
    def row(vals):
        th = np.ones(16)
        th[:len(vals)] = vals
        return th
    return {
        "m52": (K.Matern52(), row([2.0, 1.0, 1e-3])),
        "m52_ard": (K.Matern52(lengthscales=[2.0] * D), row([2.0] * D + [1.0, 1e-3])),
        "expxexp": (K.Exponential(active_dims=slice(0, D - 1)) * K.Exponential(active_dims=slice(D - 1, D)),
                    row([2.0, 1.0, 2.0, 1.0, 1e-3])),
        "expxexp_ard": (K.Exponential(lengthscales=[2.0] * (D - 1), active_dims=slice(0, D - 1))
                        * K.Exponential(active_dims=slice(D - 1, D)), row([2.0] * (D - 1) + [1.0, 2.0, 1.0, 1e-3])),
    }


def time_config(name, kernel, row, data, reps, warmup):
    b = len(data)
    eng = Engine([d[0] for d in data], [d[1] for d in data], [compile_spec(kernel, D)] * b)
    theta = np.tile(row, (b, 1))
    act = list(range(b))
    for _ in range(warmup):
        lml, _, info = eng.lml_grad(act, theta)
    assert not info.any()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        eng.lml_grad(act, theta)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    eng.ctx.set_profiling(True)
    eng.lml_grad(act, theta)
    tm = eng.last_timing()
    eng.ctx.set_profiling(False)
    out = dict(config=name, N=data[0][0].shape[0], B=b, median_ms=statistics.median(ms), min_ms=min(ms), max_ms=max(ms),
               reps=reps, factor_ms=tm.factor_ms, solve_ms=tm.alpha_ms, contract_reduce_ms=tm.grad_ms,
               lml0=float(lml[0]))
    del eng
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 32])
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    for b in args.batches:
        data = c4_data(args.n, b)
        res = {}
        for name, (kernel, row) in configs().items():
            res[name] = time_config(name, kernel, row, data, args.reps, args.warmup)
            print(json.dumps(res[name]), flush=True)
        for iso, ard in (("m52", "m52_ard"), ("expxexp", "expxexp_ard")):
            print(json.dumps(dict(B=b, pair=f"{ard}/{iso}", ratio_total=res[ard]["median_ms"] / res[iso]["median_ms"],
                                  ratio_contract=res[ard]["contract_reduce_ms"] / max(res[iso]["contract_reduce_ms"], 1e-9),
                                  ratio_factor=res[ard]["factor_ms"] / max(res[iso]["factor_ms"], 1e-9),
                                  lml_equal=res[ard]["lml0"] == res[iso]["lml0"])), flush=True)


if __name__ == "__main__":
    main()
