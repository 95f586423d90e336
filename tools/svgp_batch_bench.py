"""Time the batched small-shape SVGP path (gpx_svgp_small_*, engine.SVGPSmallEngine) at the reference's
sparse shape (n = 89, M = 20, SE kernel, days layout) on one GPU, beside the one-model path
(SVGP._elbo_and_grads -> gpx_svgp_elbo_grad) and the numpy restatement (oracle OSVGP) on the host,
and the train_svgp_model sweep (8 kernels) beside the loop of solo Scipy().minimize fits.

Every figure is the host clock around calls that end in a stream synchronise: after a warm-up,
`--windows` windows of `--reps` calls each; median [min, max] over the windows. The parts run one
after another in fresh child processes, so that no part shares the GPU with another; the one-model
parts import the package from --parent-root when given (a checkout of the parent commit with its
library built), else from this tree (whose one-model path is the parent's code, unedited).

Usage: python tools/svgp_batch_bench.py [--parent-root DIR] [--reps 200] [--windows 7] [--sweeps 5]
Prints one JSON line: the figures and the two checks
  B = 8 : the fused call's [min, max] lies below 8 x the one-model [min, max] (no overlap)
  B = 24: the fused call's median / 24 lies below the host restatement's per-evaluation median."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_ROWS, M_IND = 89, 20
BATCHES = (1, 8, 24, 432)


def days(n=N_ROWS, seed=0):
    rng = np.random.default_rng(1000 + seed)
    X = np.arange(n, dtype=np.float64)[:, None]
    y = rng.standard_normal(n)
    y = (y - y.mean()) / y.std(ddof=1)
    return X, y[:, None]


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


def _models(B, x, rng):
    import portfoliooptgp_amd as gpx
    ms = []
    for _ in range(B):
        m = gpx.models.SVGP(kernel=gpx.kernels.SquaredExponential(), likelihood=gpx.likelihoods.Gaussian(variance=1e-4),
                            inducing_variable=x[:M_IND].copy())
        gpx.set_trainable(m.likelihood.variance, False)
        R = np.tril(rng.standard_normal((M_IND, M_IND)) * 0.05)
        R[np.diag_indices(M_IND)] = rng.uniform(0.3, 1.0, M_IND)
        m.q_mu.assign(rng.standard_normal((M_IND, 1)) * 0.5)
        m.q_sqrt.assign(R[None])
        ms.append(m)
    return ms


def ref_kernels():
    import portfoliooptgp_amd as gpx
    K = gpx.kernels
    return [K.SquaredExponential(), K.Matern12(), K.RationalQuadratic(), K.Exponential(),
            K.SquaredExponential() + K.Matern12(),
            K.Exponential() + K.Periodic(K.SquaredExponential()) + K.Linear(),
            K.Exponential() + K.Periodic(K.SquaredExponential()),
            K.SquaredExponential() * K.Matern12()]


def part_fused(a):
    """The fused call for B models: `call` = gpx_svgp_small_elbo_grad alone (inputs packed), `round` =
    what the fit driver does per round (every model's state read and packed, the call, every result read)."""
    import torch
    from portfoliooptgp_amd.engine import SVGPSmallEngine
    from portfoliooptgp_amd.kernels import compile_spec
    x, y = days()
    rng = np.random.default_rng(1)
    out = {}
    for B in BATCHES:
        ms = _models(B, x, rng)
        eng = SVGPSmallEngine(B, N_ROWS, M_IND, 1)
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
    """One model on the one-model path: SVGP._elbo_and_grads (state read, gpx_svgp_elbo_grad)."""
    import torch
    import portfoliooptgp_amd as gpx
    x, y = days()
    m = _models(1, x, np.random.default_rng(1))[0]
    data = (x, y)
    return {"package": os.path.relpath(os.path.dirname(os.path.dirname(os.path.abspath(gpx.__file__))), REPO),
            "eval_ms": stats(windows(lambda: m._elbo_and_grads(data), a.reps, a.windows, torch.cuda.synchronize))}


def part_host(a):
    """The numpy restatement of the same evaluation on the host (oracle OSVGP.elbo_and_grads)."""
    from oracle import gp_oracle as O
    from oracle import svgp_oracle as S
    x, y = days()
    rng = np.random.default_rng(1)
    R = np.tril(rng.standard_normal((M_IND, M_IND)) * 0.05)
    R[np.diag_indices(M_IND)] = rng.uniform(0.3, 1.0, M_IND)
    om = S.OSVGP(O.OSquaredExponential(), x[:M_IND], num_data=N_ROWS, noise_variance=1e-4,
                 q_mu=rng.standard_normal(M_IND) * 0.5, q_sqrt=R)
    threads = int(os.environ.get("OPENBLAS_NUM_THREADS") or os.environ.get("OMP_NUM_THREADS") or os.cpu_count())
    return {"threads": threads, "eval_ms": stats(windows(lambda: om.elbo_and_grads(x, y), a.reps, a.windows, lambda: None))}


def part_sweep_batch(a):
    import torch
    from portfoliooptgp_amd.trainer import ModelTrainer
    x, y = days()
    ts, mse, nfev = [], None, None
    for _ in range(a.sweeps + 1):  # (the first run warms up)
        tr = ModelTrainer(ref_kernels())
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        _, mse, _ = tr.train_svgp_model(x, y, n_inducing=M_IND, maxiter=100)
        ts.append(time.perf_counter() - t0)
        nfev = [int(r.nfev) for r in tr.last_results]
    return {"seconds": stats(ts[1:], 1.0), "best_mse": mse, "nfev": nfev}


def part_sweep_solo(a):
    import torch
    import portfoliooptgp_amd as gpx
    from portfoliooptgp_amd.trainer import mean_squared_error
    x, y = days()
    ts, best, nfev = [], None, None
    for _ in range(a.sweeps + 1):
        ks = ref_kernels()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        best, nfev = float("inf"), []
        for k in ks:
            m = gpx.models.SVGP(kernel=k, likelihood=gpx.likelihoods.Gaussian(variance=1e-4),
                                inducing_variable=x[:M_IND].copy())
            gpx.set_trainable(m.likelihood.variance, False)
            r = gpx.optimizers.Scipy().minimize(m.training_loss_closure((x, y)), m.trainable_variables,
                                                options=dict(maxiter=100))
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
    ap.add_argument("--sweeps", type=int, default=5, help="timed train_svgp_model sweeps (after one warm-up)")
    ap.add_argument("--part", default=None, choices=sorted(PARTS))
    ap.add_argument("--part-timeout", type=int, default=240, help="seconds a part may take")
    a = ap.parse_args()
    if a.part:
        sys.path.insert(0, a.root or REPO)
        print(json.dumps(PARTS[a.part](a)))
        return
    out = {"shape": {"n": N_ROWS, "M": M_IND, "kernel": "SE", "layout": "days"}, "reps": a.reps, "windows": a.windows}
    for part in ("solo", "fused", "host", "sweep_solo", "sweep_batch"):
        out[part] = child(part, a, a.parent_root if part in ("solo", "sweep_solo") else None)
        if "error" in out[part]:  # nothing more is started on the GPU after a failed part
            print(json.dumps(out))
            sys.exit(1)
    solo, host, fused = out["solo"]["eval_ms"], out["host"]["eval_ms"], out["fused"]
    out["check_B8_below_8x_solo"] = fused["8"]["call_ms"]["max"] < 8 * solo["min"]
    out["check_B24_per_model_below_host"] = fused["24"]["call_ms"]["median"] / 24 < host["median"]
    out["speedup_call_vs_solo"] = {B: int(B) * solo["median"] / fused[B]["call_ms"]["median"] for B in fused}
    out["speedup_round_vs_solo"] = {B: int(B) * solo["median"] / fused[B]["round_ms"]["median"] for B in fused}
    out["sweep_speedup"] = out["sweep_solo"]["seconds"]["median"] / out["sweep_batch"]["seconds"]["median"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
