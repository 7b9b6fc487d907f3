"""N > 1 path on CPU: bench.py's sharding logic under torch.distributed with the gloo backend, world_size 2.
Windows are independent, so ranks only meet at the barrier and the max-over-ranks reduction; this test checks that the
per-rank seed partition is disjoint and that the collective plumbing works (no GPU, no solver call)."""
import os
import subprocess
import sys
import textwrap

from conftest import ROOT

WORKER = textwrap.dedent("""
    import os, sys, json
    sys.path.insert(0, %r)
    import torch, torch.distributed as dist
    from cerberus_amd import synth
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    dist.init_process_group("gloo", rank=rank, world_size=world)
    W = 3
    cfg = synth.default_config()
    seeds = [20260925 + rank * W + i for i in range(W)]            # bench.py's partition
    ws = [synth.make_window(cfg, n_landmarks=12, seed=s) for s in seeds]
    sig = torch.tensor([float(w.obs.sum()) for w in ws], dtype=torch.float64)
    allsig = [torch.zeros(W, dtype=torch.float64) for _ in range(world)]
    dist.all_gather(allsig, sig)
    t = torch.tensor([1.0 + rank], dtype=torch.float64)
    dist.barrier()
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    if rank == 0:
        flat = torch.cat(allsig).tolist()
        print(json.dumps({"max_time": t.item(), "distinct": len(set(flat)), "n": len(flat), "seeds": seeds}))
    dist.destroy_process_group()
""") % ROOT


def test_two_rank_gloo_sharding(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29531")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29531", str(script)], capture_output=True, text=True, timeout=300, env=env)
    assert out.returncode == 0, out.stderr[-2000:]
    import json
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    res = json.loads(line)
    assert res["max_time"] == 2.0          # max over ranks
    assert res["distinct"] == res["n"] == 6  # every rank solved different windows


import pytest


@pytest.mark.gpu
def test_bench_py_itself_on_two_ranks_of_one_gpu():
    """The real bench.py under torch.distributed.run with two ranks sharing the one GPU of the test box (VILO_BENCH_BACKEND=gloo,
    local_rank % device_count): the N > 1 code path of the script the driver launches — rank-disjoint windows, barrier + max-over-ranks
    timing, whole-job value."""
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29533", VILO_BENCH_BACKEND="gloo")
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29533", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--windows", "64",
                          "--full", "--no-cpu-baseline", "--no-single-window"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["scaling"] == "weak" and d["steps"] == 2
    W, it = d["config"]["windows_per_gpu"], d["config"]["iterations_per_step"]
    assert W == 64 and d["config"]["total_windows"] == 128
    assert abs(d["value"] - 2 * W * it / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    sh = d["config"]["shards"]
    assert len(sh) == 2 and sh[0][1] < sh[1][0] and sh[0][2] != sh[1][2]   # disjoint seed ranges, different data
    # the strong-scaling side block of the default (weak) mode: BASELINE configs[3]'s 1024 windows in total, 512 per rank here
    ss = d["strong_scaling"]
    assert ss["scaling"] == "strong" and ss["total_windows"] == 1024 and ss["windows_per_gpu"] == 512 and ss["n_gpus"] == 2
    assert abs(ss["value"] - 1024 * it / (ss["ms_per_step"] * 1e-3)) < 1e-6 * ss["value"]
    # BASELINE configs[3] mode: a fixed total, window w on rank w mod 2
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29534", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--total-windows", "64",
                          "--no-cpu-baseline", "--no-single-window"], capture_output=True, text=True, timeout=900,
                         env=dict(env, MASTER_PORT="29534"), cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["scaling"] == "strong" and d["config"]["windows_per_gpu"] == 32 and d["config"]["total_windows"] == 64
    assert abs(d["value"] - 64 * it / (d["ms_per_step"] * 1e-3)) < 1e-6 * d["value"]
    sh = d["config"]["shards"]
    assert sh[0][0] + 1 == sh[1][0]   # interleaved: w mod 2
    assert d["ranks_in_process_group"] == 2 and abs(d["value_per_gpu"] * 2 - d["value"]) < 1e-9 * d["value"]
    # the same WITHOUT a launcher: `python bench.py --gpus 2` starts its two ranks itself (a bare invocation must not measure one GPU
    # and call it two)
    bare = {k: v for k, v in env.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--total-windows", "64",
                          "--no-cpu-baseline", "--no-single-window"], capture_output=True, text=True, timeout=900, env=bare, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["ranks_in_process_group"] == 2 and d["config"]["windows_per_gpu"] == 32


def test_bench_py_refuses_a_world_size_that_is_not_its_gpus_flag():
    """`--gpus N` is checked against the ranks the launcher started (before anything touches a device): one rank can never be reported as
    N GPUs, nor N ranks as one."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                         timeout=120, env=env, cwd=ROOT)
    assert out.returncode == 2 and "WORLD_SIZE=1" in out.stderr
    env = dict(os.environ, WORLD_SIZE="2", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0"], capture_output=True, text=True,
                         timeout=120, env=env, cwd=ROOT)
    assert out.returncode == 2


CONTROL_WORKER = textwrap.dedent("""
    import os, sys, json
    sys.path.insert(0, %r)
    import bench
    rank, world = int(os.environ["RANK"]), int(os.environ["WORLD_SIZE"])
    ctl = bench.init_control_plane(rank, world, 0, want="nccl", probe_timeout_s=60.0)   # no GPU here: the RCCL probe must fail on every rank
    ctl.barrier(0)
    t = ctl.max_over_ranks(1.0 + rank, 0)
    sh = ctl.all_gather([float(rank), float(10 + rank)], 0, world)
    if rank == 0:
        print(json.dumps({"backend": ctl.backend, "note": ctl.note, "max": t, "shards": sh}))
    sys.stdout.flush()
    os._exit(0)
""") % ROOT


def test_control_plane_falls_back_to_gloo_when_rccl_cannot_start(tmp_path):
    """bench.py's control collectives (barrier, max-over-ranks, shard report): gloo is the default process group, RCCL is probed and the
    ranks agree over gloo whether every probe succeeded. Without a GPU the probe fails on both ranks: the three calls must run over gloo."""
    import json
    script = tmp_path / "ctl_worker.py"
    script.write_text(CONTROL_WORKER)
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29537")
    env.pop("VILO_BENCH_BACKEND", None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29537", str(script)], capture_output=True, text=True, timeout=600, env=env)
    assert out.returncode == 0, out.stderr[-3000:]
    res = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert res["backend"] == "gloo" and "RCCL unavailable" in res["note"]
    assert res["max"] == 2.0 and res["shards"] == [[0.0, 10.0], [1.0, 11.0]]


@pytest.mark.gpu
def test_bench_py_survives_an_rccl_that_cannot_start():
    """Two ranks on the ONE GPU of the test box with the default backend: RCCL refuses ("Duplicate GPU detected" — how round 4's only attempt
    at the nccl leg died). The line must still come out, over gloo, with the contract fields an N > 1 line needs."""
    import json
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29539")
    env.pop("VILO_BENCH_BACKEND", None)
    out = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                          "--master-port", "29539", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "2", "--warmup", "1", "--windows", "64",
                          "--full", "--no-single-window", "--no-strong", "--no-replay", "--no-config3"], capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-3000:]
    d = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["ranks_in_process_group"] == 2
    assert d["control_backend"] == "gloo" and "RCCL unavailable" in d["control_backend_note"]
    assert d["cpu_baseline"] and d["cpu_baseline"]["cores"] == 1 and d["cpu_baseline"]["value"] > 0      # rank 0 times it at N > 1 too
    assert d["roofline"]["frac"] > 0 and d["parity_sample"]["max_state_err"] < d["parity_sample"]["tolerance"]
