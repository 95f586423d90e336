"""Time the batched small-shape SGPR path (gpx_sgpr_small_*, engine.SGPRSmallEngine) at the reference's
SGPR shape (n = 113, M = 10, SE kernel, inducing points on a linspace grid) on one GPU, beside the
one-model path (SGPR._elbo_and_grads -> gpx_sgpr_elbo_grad) and the numpy restatement
(tests/sgpr_numpy.NumpySGPR) on the host, and the train_sgpr_model sweep (8 kernels) beside the loop
of solo Scipy().minimize fits + predict_f.

Every figure is the host clock around calls that end in a stream synchronise: after a warm-up,
`--windows` windows of `--reps` calls each; median [min, max] over the windows. The parts run one
after another in fresh child processes, so that no part shares the GPU with another; the one-model
parts import the package from --parent-root when given (a checkout of the parent commit with its
library built), else from this tree (whose one-model path is the parent's code, unedited).

Usage: python tools/sgpr_batch_bench.py [--parent-root DIR] [--reps 200] [--windows 7] [--sweeps 5]
Prints one JSON line: the figures and the three conditions, each judged by [min, max] intervals
  (a) B = 8 : the fused call's max lies below 8 x the one-model min
  (b) B = 24: the fused call's max / 24 lies below the host restatement's min
  (c) B = 1 : "faster" when the fused call's max lies below the one-model min, "slower" when its min
              lies above the one-model max, "overlap" otherwise."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_ROWS, M_IND = 113, 10
BATCHES = (1, 8, 24, 432)


def cell(n=N_ROWS, seed=6):
    """tests/test_sgpr_gpu.py's "ref" case: uniform X in [0, 10], a noisy sine, Z = linspace(0, 10, M)."""
    rng = np.random.default_rng(seed)
    X = rng.uniform(0, 10, (n, 1))
    Y = np.sin(X) + 0.3 * np.cos(2 * X) + 0.05 * rng.standard_normal((n, 1))
    return X, Y, np.linspace(0, 10, M_IND)[:, None]


def stats(ts, scale=1e3):
    return {"median": statistics.median(ts) * scale, "min": min(ts) * scale, "max": max(ts) * scale}


def windows(fn, reps, nwin, sync):
    for _ in range(max(3, reps // 10)):
        fn()
    out = []
    for _ in range(nwin):
        sync()
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        sync()
        out.append((time.perf_counter() - t0) / reps)
    return out


def ref_kernels():
    import portfoliooptgp_amd as gpx
    K = gpx.kernels
    return [K.SquaredExponential(), K.Matern12(), K.RationalQuadratic(), K.Exponential(),
            K.SquaredExponential() + K.Matern12(),
            K.Exponential() + K.Periodic(K.SquaredExponential()) + K.Linear(),
            K.Exponential() + K.Periodic(K.SquaredExponential()),
            K.SquaredExponential() * K.Matern12()]


def part_fused(a):
    """The fused call for B models: `call` = gpx_sgpr_small_elbo_grad alone (inputs packed), `round` =
    what the fit driver does per round (every model's state read and packed, the call, every result read)."""
    import torch
    import portfoliooptgp_amd as gpx
    from portfoliooptgp_amd.engine import SGPRSmallEngine
    from portfoliooptgp_amd.kernels import compile_spec
    x, y, z = cell()
    out = {}
    for B in BATCHES:
        ms = [gpx.models.SGPR((x, y), gpx.kernels.SquaredExponential(), inducing_variable=z.copy()) for _ in range(B)]
        eng = SGPRSmallEngine(B, N_ROWS, M_IND, 1)
        for b, m in enumerate(ms):
            eng.bind(b, x, y, compile_spec(m.kernel, 1), M_IND)
            eng.pack(b, *m._state())
        act = list(range(B))
        reps = a.reps if B < 100 else max(20, a.reps // 4)

        def rnd():
            for b, m in enumerate(ms):
                eng.pack(b, *m._state())
            eng.elbo_grad(act)
            for b in act:
                eng.result(b)
        out[str(B)] = {"reps": reps, "call_ms": stats(windows(lambda: eng.elbo_grad(act), reps, a.windows, torch.cuda.synchronize)),
                       "round_ms": stats(windows(rnd, reps, a.windows, torch.cuda.synchronize))}
    return out


def part_solo(a):
    """One model on the one-model path: SGPR._elbo_and_grads (state read, gpx_sgpr_elbo_grad)."""
    import torch
    import portfoliooptgp_amd as gpx
    x, y, z = cell()
    m = gpx.models.SGPR((x, y), gpx.kernels.SquaredExponential(), inducing_variable=z)
    return {"package": os.path.relpath(os.path.dirname(os.path.dirname(os.path.abspath(gpx.__file__))), REPO),
            "eval_ms": stats(windows(m._elbo_and_grads, a.reps, a.windows, torch.cuda.synchronize))}


def part_host(a):
    """The numpy restatement of the same evaluation on the host (NumpySGPR.elbo_and_grads, GPflow's route)."""
    from oracle import gp_oracle as O
    from tests.sgpr_numpy import NumpySGPR
    x, y, z = cell()
    om = NumpySGPR(O.OSquaredExponential(), x, y, z, noise_variance=1.0)
    threads = int(os.environ.get("OPENBLAS_NUM_THREADS") or os.environ.get("OMP_NUM_THREADS") or os.cpu_count())
    return {"threads": threads, "eval_ms": stats(windows(om.elbo_and_grads, a.reps, a.windows, lambda: None))}


def part_sweep_batch(a):
    import torch
    from portfoliooptgp_amd.trainer import ModelTrainer
    x, y, _ = cell()
    ts, mse, nfev = [], None, None
    for _ in range(a.sweeps + 1):  # (the first run warms up)
        tr = ModelTrainer(ref_kernels())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, mse, _ = tr.train_sgpr_model(x, y, n_inducing=M_IND, maxiter=100)
        ts.append(time.perf_counter() - t0)
        nfev = [int(r.nfev) for r in tr.last_results]
    return {"seconds": stats(ts[1:], 1.0), "best_mse": mse, "nfev": nfev}


def part_sweep_solo(a):
    import torch
    import portfoliooptgp_amd as gpx
    from portfoliooptgp_amd.trainer import mean_squared_error
    x, y, _ = cell()
    z = np.linspace(x.min(), x.max(), M_IND)[:, None]  # train_sgpr_model's layout
    ts, best, nfev = [], None, None
    for _ in range(a.sweeps + 1):
        ks = ref_kernels()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best, nfev = float("inf"), []
        for k in ks:
            m = gpx.models.SGPR((x, y), k, inducing_variable=z.copy())
            r = gpx.optimizers.Scipy().minimize(m.training_loss, m.trainable_variables, options=dict(maxiter=100))
            nfev.append(int(r.nfev))
            best = min(best, mean_squared_error(y, m.predict_f(x)[0].numpy()))
        ts.append(time.perf_counter() - t0)
    return {"package": os.path.relpath(os.path.dirname(os.path.dirname(os.path.abspath(gpx.__file__))), REPO),
            "seconds": stats(ts[1:], 1.0), "best_mse": best, "nfev": nfev}


PARTS = {"fused": part_fused, "solo": part_solo, "host": part_host, "sweep_batch": part_sweep_batch,
         "sweep_solo": part_sweep_solo}


def child(part, a, root=None):
    cmd = [sys.executable, os.path.abspath(__file__), "--part", part, "--reps", str(a.reps), "--windows", str(a.windows),
           "--sweeps", str(a.sweeps), "--root", os.path.abspath(root or REPO)]
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.part_timeout)
    if r.returncode != 0:
        return {"error": f"exit {r.returncode}", "stderr": r.stderr[-600:]}
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None,
                    help="a checkout of the parent commit with its library built: the one-model parts import it")
    ap.add_argument("--root", default=None, help="(a part's child process) the tree to import the package from")
    ap.add_argument("--reps", type=int, default=200, help="calls per timing window")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--sweeps", type=int, default=5, help="timed train_sgpr_model sweeps (after one warm-up)")
    ap.add_argument("--part", default=None, choices=sorted(PARTS))
    ap.add_argument("--part-timeout", type=int, default=240, help="seconds a part may take")
    a = ap.parse_args()
    if a.part:
        sys.path.insert(0, a.root or REPO)
        print(json.dumps(PARTS[a.part](a)))
        return
    out = {"shape": {"n": N_ROWS, "M": M_IND, "kernel": "SE", "layout": "grid"}, "reps": a.reps, "windows": a.windows}
    for part in ("solo", "fused", "host", "sweep_solo", "sweep_batch"):
        out[part] = child(part, a, a.parent_root if part in ("solo", "sweep_solo") else None)
        if "error" in out[part]:  # nothing more is started on the GPU after a failed part
            print(json.dumps(out))
            sys.exit(1)
    solo, host, fused = out["solo"]["eval_ms"], out["host"]["eval_ms"], out["fused"]
    out["cond_a_B8_below_8x_solo"] = fused["8"]["call_ms"]["max"] < 8 * solo["min"]
    out["cond_b_B24_per_model_below_host"] = fused["24"]["call_ms"]["max"] / 24 < host["min"]
    f1 = fused["1"]["call_ms"]
    out["cond_c_B1_vs_solo"] = "faster" if f1["max"] < solo["min"] else "slower" if f1["min"] > solo["max"] else "overlap"
    out["speedup_call_vs_solo"] = {B: int(B) * solo["median"] / fused[B]["call_ms"]["median"] for B in fused}
    out["speedup_round_vs_solo"] = {B: int(B) * solo["median"] / fused[B]["round_ms"]["median"] for B in fused}
    out["sweep_speedup"] = out["sweep_solo"]["seconds"]["median"] / out["sweep_batch"]["seconds"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
