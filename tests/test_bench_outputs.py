"""bench.py's options around the timed region: --full is off by default and gates the CPU baseline
and the secondary lines' flags; --dump-outputs writes the host processes' last-step outputs in
process order as float64 .npy; the threaded series generator returns what lone calls return."""
import os

import numpy as np

import bench


def test_plain_run_is_the_default():
    a = bench.parse_args([])
    assert a.full is False and a.dump_outputs is None
    a = bench.parse_args(["--gpus", "1", "--steps", "3", "--warmup", "1", "--full", "--dump-outputs", "d"])
    assert a.full is True and a.dump_outputs == "d" and a.steps == 3 and a.warmup == 1
    assert not a.no_cpu_baseline and not a.no_secondary


def test_write_outputs_orders_processes_and_offsets_rows(tmp_path):
    n = 7
    rng = np.random.default_rng(0)

    def part(w, rows, pick):
        return (w, rng.standard_normal((rows, 6)), np.asarray(pick), rng.standard_normal((len(pick), n)),
                rng.uniform(0.1, 1.0, (len(pick), n)).astype(np.float32))
    p0, p1, p2 = part(0, 5, [1, 4]), part(1, 4, [0, 3]), part(2, 4, [2])
    out = str(tmp_path / "dump")
    bench.write_outputs(out, [p2, p0, p1])  # (helpers answer in any order)
    assert sorted(os.listdir(out)) == ["fit_summary.npy", "predict_fit_index.npy", "predict_mean.npy",
                                       "predict_var.npy"]
    got = {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}
    assert all(a.dtype == np.float64 for a in got.values())
    assert np.array_equal(got["fit_summary"], np.concatenate([p0[1], p1[1], p2[1]]))
    assert np.array_equal(got["predict_fit_index"], [1, 4, 5, 8, 11])
    assert np.array_equal(got["predict_mean"], np.concatenate([p0[3], p1[3], p2[3]]))
    assert np.array_equal(got["predict_var"], np.concatenate([p0[4], p1[4], p2[4]]).astype(np.float64))
    # the sampled rows belong to the summary rows they name
    assert got["predict_mean"].shape == (5, n) and got["predict_fit_index"].max() < len(got["fit_summary"])


def test_series_batch_equals_lone_calls():
    seeds = [0, 3, 11, 12, 500]
    lone = [bench.synthetic_series(96, s) for s in seeds]
    for procs in (1, 8, 10 ** 6):  # (several threads where the CPUs allow; one thread)
        got = bench.series_batch(96, seeds, procs)
        assert len(got) == len(seeds)
        for (x, y), (x0, y0) in zip(got, lone):
            assert np.array_equal(x, x0) and np.array_equal(y, y0)
