"""ms per vilo_batch_leg_dead_reckon call (GPU time of k_leg_dead_reckon, HIP events, after a warm-up; with and without the trajectory)
next to vilo_batch_dead_reckon on the same batch and samples and vilo_preintegrate over the same intervals, from the same run, at 128,
4096 and 32768 config-2 windows with 30 samples each. The state is the one a solve leaves. The host's packing and upload of the samples
and the copies out are outside the two calls' GPU time; wall_ms is the whole Python call. vilo_preintegrate is a host-pointer call without
an event timer of its own: its figure is the wall time of the call, upload of the samples and download of the 15.6 KB records included,
and is marked so.
    python tools/time_leg_dead_reckon.py [--sizes 128,4096,32768] [--samples 30] [--reps 5] > profiles/leg_dead_reckon_time.txt"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,4096,32768")
    ap.add_argument("--samples", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from cerberus_amd import api, synth
    cfg = synth.default_config()
    ctx = api.Context(cfg, 0)
    base = synth.make_window(cfg, params=synth.default_params(config=2, seed=20260925))
    ctx.preintegrate_window(base)
    lib = api.lib()
    for W in [int(s) for s in a.sizes.split(",")]:
        b = api.Batch(ctx, [base.twin() for _ in range(W)])
        b.solve(api.default_solve_opts(True, 4))
        b.download()
        # window i reads a.samples rows of the generated stream from row i % 64 on: neighbouring quads do not read the same bytes
        samples = np.ascontiguousarray(np.concatenate([base.samples[i % 64:i % 64 + a.samples] for i in range(W)]))
        offsets = np.arange(W + 1, dtype=np.int32) * a.samples
        f = base.F - 1
        lin = np.ascontiguousarray(np.tile(np.concatenate([base.speed_bias[f, 3:9], base.leg_bias[f]]), (W, 1)))
        r = b.leg_dead_reckon(samples, offsets, trajectory=True)   # (warm-up: the first call takes its arena chunks from the device)
        b.dead_reckon(samples, offsets)
        ctx.preintegrate(samples, offsets, lin)
        ms = {"state": [], "trajectory": [], "imu": [], "preint_wall": []}
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            b.leg_dead_reckon(samples, offsets)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms["state"].append(lib.vilo_last_leg_dead_reckon_ms(ctx.h))
            b.leg_dead_reckon(samples, offsets, trajectory=True)
            ms["trajectory"].append(lib.vilo_last_leg_dead_reckon_ms(ctx.h))
            b.dead_reckon(samples, offsets)
            ms["imu"].append(lib.vilo_last_dead_reckon_ms(ctx.h))
            t0 = time.perf_counter()
            ctx.preintegrate(samples, offsets, lin)
            ms["preint_wall"].append(1e3 * (time.perf_counter() - t0))
        s_ms = min(ms["state"])
        print(json.dumps({"windows": W, "samples_per_window": a.samples, "steps": int(r.n_steps.sum()), "status_ok": int((r.status == 0).sum()),
                          "leg_dead_reckon_gpu_ms": round(s_ms, 4), "leg_dead_reckon_trajectory_gpu_ms": round(min(ms["trajectory"]), 4),
                          "dead_reckon_gpu_ms": round(min(ms["imu"]), 4), "preintegrate_wall_ms": round(min(ms["preint_wall"]), 3),
                          "leg_dead_reckon_wall_ms": round(min(wall), 3), "ns_per_step": round(1e6 * s_ms / max(1, int(r.n_steps.sum())), 3),
                          "packed_bytes": int(280 * len(samples)), "ratio_to_dead_reckon": round(s_ms / min(ms["imu"]), 3)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
