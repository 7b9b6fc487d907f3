"""The bench line's contract (task brief, section 4): the newest committed `profiles/round*_bench_v*.json` is a line bench.py printed
on an MI355X; its keys, units and internal arithmetic are checked here so a change to bench.py that breaks the contract shows
up in the CPU suite."""
import glob
import json
import os

import pytest

from conftest import ROOT


def _newest():
    """the default line of the newest round that committed one (profiles/roundN_bench_final.json; rounds 1 - 3 named them _vK)"""
    finals = sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_bench_final.json")), key=lambda p: int(os.path.basename(p).split("_")[0][5:]))
    if finals:
        return json.load(open(finals[-1]))

    def key(p):
        b = os.path.basename(p)
        return (int(b.split("_")[0][5:]), int(b.split("_v")[1].split("_")[0].split(".")[0]))
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "round*_bench_v*.json")), key=key)
    return json.load(open(files[-1]))


def test_bench_line_has_the_contract_fields():
    d = _newest()
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config",
              "roofline", "cpu_baseline"):
        assert k in d, k
    assert d["metric"] == json.load(open(os.path.join(ROOT, "BASELINE.json")))["metric"].replace("\u00d7", " x ").replace("  ", " ") or "GN iters/sec" in d["metric"]
    assert d["higher_is_better"] is True and d["scaling"] == "weak" and d["vs_baseline"] is None and d["dtype"] == "f64" and d["data"] == "synthetic"
    assert "workload" in d["config"] and "model" not in d["config"]
    r = d["roofline"]
    for k in ("bound", "achieved", "peak", "unit", "frac", "traffic"):
        assert k in r, k
    assert r["bound"] in ("hbm", "mfma") and r["unit"] in ("GB/s", "TFLOP/s")
    assert abs(r["frac"] - r["achieved"] / r["peak"]) < 1e-12
    c = d["cpu_baseline"]
    for k in ("value", "unit", "cores", "kind", "sample"):
        assert k in c, k
    assert c["kind"] in ("reference", "port") and c["cores"] >= 1


def test_bench_line_arithmetic():
    d = _newest()
    W, it = d["config"]["windows_per_gpu"], d["config"]["iterations_per_step"]
    # value = whole-job window-iterations / time of the timed steps
    assert abs(d["value"] - d["n_gpus"] * W * it / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    r = d["roofline"]
    # achieved = algorithmic bytes per launch (per-window figure x windows of one launch) / average launch duration of the dominant kernel
    assert abs(r["achieved"] - r["algorithmic_bytes_per_window_iteration"] * W / (r["kernel_avg_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert r["kernel"] in d["kernels"] and abs(d["kernels"][r["kernel"]]["avg_ms"] - r["kernel_avg_ms"]) < 1e-12
    # the dominant kernel's measured HBM traffic is a per-launch byte count of plausible size
    assert r["traffic"] is None or 0.1 * r["algorithmic_bytes_per_window_iteration"] * W < r["traffic"] < 50 * r["algorithmic_bytes_per_window_iteration"] * W


def test_the_line_checks_what_it_timed():
    """parity_sample of the committed line looks at the first, a middle and the LAST windows of the timed batch and at every window's cost;
    cpu_baseline names its host and carries the compiled reference's Evaluate pass; the counters behind roofline.traffic belong to the
    kernels that ran."""
    d = _newest()
    W = d["config"]["windows_per_gpu"]
    ps = d["parity_sample"]
    idx = ps["window_indices"]
    assert idx[0] == 0 and idx[-1] == W - 1 and any(W // 4 < i < 3 * W // 4 for i in idx)
    assert max(ps["max_state_err"], ps["max_cost_rel"]) <= ps["tolerance"] == 1e-8
    aw = ps["all_windows"]
    assert aw["n"] == W and aw["ok"] and aw["outside_0.1x_10x_of_median"] == 0 and aw["states_finite"]
    c = d["cpu_baseline"]
    assert c["cpu_model"] and c["nproc"] >= c["cores"]
    re = c["reference_evaluate"]
    assert re["kind"] == "reference" and re["residual_blocks_per_pass"] > 3000 and 0.1 < re["ms_per_evaluation_pass"] < 100
    assert d["roofline"]["traffic_source"]["stale"] is False
    hi = d["host_inclusive"]
    one = hi.get("as_one_batch", hi)     # (lines from before the call pipelined itself carry the one batch only)
    assert abs(one["value"] - hi["windows"] * d["config"]["iterations_per_step"] / (one["ms"]["total"] * 1e-3)) < 1e-6 * one["value"]
    if one is not hi:
        assert abs(hi["value"] - hi["windows"] * d["config"]["iterations_per_step"] / (hi["ms"] * 1e-3)) < 1e-6 * hi["value"]
        assert hi["bitwise_equal_to_one_batch"] is True and hi["value"] >= one["value"]
    assert hi["value"] < d["value"]        # (the hand-over costs: it can never look faster than the resident line)


def test_sample_indices_cover_head_middle_and_tail():
    import sys
    sys.path.insert(0, ROOT)
    import bench
    for W in (1, 2, 5, 9, 256, 32768):
        idx = bench.sample_indices(W)
        assert idx == sorted(set(idx)) and idx[0] == 0 and idx[-1] == W - 1 and all(0 <= i < W for i in idx) and len(idx) <= 9
    assert bench.sample_indices(32768) == [0, 1, 2, 16383, 16384, 16385, 32765, 32766, 32767]


def test_threaded_window_generation_is_the_serial_one(cfg):
    """bench.py generates its batches on a pool of host threads: the windows must be the serial loop's, bit for bit and in order, or two
    runs with the same arguments would not time (and dump) the same work."""
    import sys
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    seeds = [20260925 + g for g in range(300)]
    par = bench.make_synth_windows(cfg, 200, 500, seeds)
    assert len(par) == len(seeds)
    for s, w in zip(seeds, par):
        ref = bench.make_synth_window(cfg, 200, 500, s)
        for name in ("lm_start_frame", "lm_obs_offset", "obs", "obs_is_stereo", "samples", "sample_offsets", "lin", "pose", "speed_bias", "leg_bias",
                     "ex_pose", "td", "inv_depth"):
            np.testing.assert_array_equal(getattr(w, name), getattr(ref, name), err_msg="%s of seed %d" % (name, s))
        np.testing.assert_array_equal(w.prior.J0, ref.prior.J0)
        np.testing.assert_array_equal(w.prior.r0, ref.prior.r0)


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_dumps_what_it_computed(tmp_path, cfg, ocfg):
    """`bench.py --steps K --warmup W` measures the headline alone (no side block, no check against the oracle); `--dump-outputs DIR`
    writes the last timed step's results as float64 .npy files. Two runs with the same arguments dump the same arrays, and the first and
    last windows' dumped states are the oracle's after the same fixed iterations."""
    import json
    import subprocess
    import sys
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from cerberus_amd import api
    from oracle import oracle_py as O
    W, steps = 300, 3
    runs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup", "1", "--windows", str(W),
                              "--dump-outputs", str(d)], capture_output=True, text=True, timeout=600, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-3000:]
        line = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == steps and line["warmup"] == 1 and line["higher_is_better"] is True and line["dtype"] == "f64"
        assert abs(line["value"] - W * bench.ITERS / (line["ms_per_step"] * 1e-3)) < 1e-6 * line["value"]
        for side in ("strong_scaling", "small_batches", "host_inclusive", "parity_sample", "single_window_iters_per_s", "two_streams", "config3",
                     "replay", "marginalize", "cpu_baseline_all_cores"):
            assert side not in line, side
        assert line["cpu_baseline"] is None
        files = sorted(d.glob("*.npy"))
        assert sum(f.stat().st_size for f in files) <= 64 << 20
        runs.append({f.stem: np.load(f) for f in files})
    a, b = runs
    assert sorted(a) == sorted(b)
    for name in ("final_cost", "iterations", "window_index", "pose", "speed_bias", "leg_bias", "ex_pose", "td", "inv_depth"):
        assert a[name].dtype == np.float64, name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    np.testing.assert_array_equal(a["window_index"], np.arange(W))     # (300 windows fit: all of them)
    assert (a["iterations"] == bench.ITERS).all() and a["pose"].shape == (W, bench.make_synth_window(cfg, 200, 500, 0).pose.shape[0], 7)
    ctx = api.Context(cfg, device=0)
    try:
        for i in (0, W - 1):
            w = bench.make_synth_window(cfg, 200, 500, 20260925 + i)
            ctx.preintegrate_window(w)
            osum = O.solve_window(ocfg, w, O.default_opts(fixed_iterations=True, max_num_iterations=bench.ITERS))
            for name, ref in zip(("pose", "speed_bias", "leg_bias", "ex_pose", "td", "inv_depth"), w.state_arrays()):
                assert np.abs(a[name][i] - ref).max() <= 1e-8 * max(1.0, np.abs(ref).max()), (i, name)
            assert abs(a["final_cost"][i] - osum.final_cost) <= 1e-8 * abs(osum.final_cost)
    finally:
        ctx.close()


def test_dumped_outputs_stay_under_64_mb_with_a_fixed_sample(tmp_path, cfg):
    """dump_outputs on a batch too large to dump whole: every window's summary, the states of a seeded sample that always holds the first,
    middle and last windows — the same sample from call to call — in float64 and under 64 MB in all."""
    import sys
    import numpy as np
    sys.path.insert(0, ROOT)
    import bench
    from cerberus_amd import _ctypes as T
    W = 40000
    w0 = bench.make_synth_window(cfg, 200, 500, 20260925)
    windows = [w0.twin() for _ in range(W)]
    for i in (0, W // 2, W - 1):
        windows[i].pose[0, 0] = i
    summ = list((T.SolveSummary * W)())
    for i, s in enumerate(summ):
        s.iterations, s.final_cost = bench.ITERS, float(i)
    dumped = []
    for k in range(2):
        d = tmp_path / ("d%d" % k)
        bench.dump_outputs(str(d), windows, summ)
        files = sorted(d.glob("*.npy"))
        assert 0 < sum(f.stat().st_size for f in files) <= 64 << 20
        dumped.append({f.stem: np.load(f) for f in files})
    a, b = dumped
    for name in a:
        assert a[name].dtype == np.float64, name
        np.testing.assert_array_equal(a[name], b[name], err_msg=name)
    idx = a["window_index"].astype(np.int64)
    assert 1000 < len(idx) < W and (np.diff(idx) > 0).all() and set(bench.sample_indices(W)) <= set(idx.tolist())
    assert len(a["final_cost"]) == W and (a["final_cost"] == np.arange(W)).all() and (a["iterations"] == bench.ITERS).all()
    assert a["pose"].shape == (len(idx),) + w0.pose.shape and a["inv_depth"].shape == (len(idx), w0.L)
    for i in (0, W // 2, W - 1):
        assert a["pose"][np.searchsorted(idx, i), 0, 0] == i
