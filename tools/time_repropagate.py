"""ms per vilo_batch_repropagate call (GPU time, HIP events: k_reprop_point and, with write, the integration, k_reprop_commit and the
preparation) at 128, 4096 and 32768 config-2 windows: the drift query, every interval, and the DRIFTED selection with half of the windows
away from their records' point. Beside it a 12-iteration solve on fixed records and the same solve with vilo_batch_set_samples in force.
The uploads of the samples and the copies out are outside the GPU time; wall_ms is the whole Python call, uploads included. Reported,
not gated.
    python tools/time_repropagate.py [--sizes 128,4096,32768] [--reps 3] > profiles/repropagate_time.txt"""
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
    ap.add_argument("--reps", type=int, default=3)
    a = ap.parse_args()
    from cerberus_amd import api, synth
    cfg = synth.default_config()
    ctx = api.Context(cfg, 0)
    base = synth.make_window(cfg, params=synth.default_params(config=2, seed=20260925))
    ctx.preintegrate_window(base)
    moved = base.twin()   # biases 0.2 m/s^2 / 0.02 rad/s / 0.02 m from the records' point: above the default thresholds
    moved.speed_bias[:, 3:6] += 0.2
    moved.speed_bias[:, 6:9] += 0.02
    moved.leg_bias += 0.02
    lib = api.lib()
    opts = api.default_solve_opts(True, 12)
    n1 = int(base.sample_offsets[-1])
    for W in [int(s) for s in a.sizes.split(",")]:
        ws = [(moved if i % 2 else base).twin() for i in range(W)]
        b = api.Batch(ctx, ws)
        samples = np.ascontiguousarray(np.tile(base.samples[:n1], (W, 1)))
        offsets = np.ascontiguousarray(np.concatenate([[0], (base.sample_offsets[1:][None, :] + n1 * np.arange(W)[:, None]).reshape(-1)]), dtype=np.int32)
        b.solve(opts)
        b.reset()
        fixed_ms = b.solve(opts)
        b.reset()
        b.repropagate(samples, offsets)   # (warm-up: the first call takes its arena chunks from the device)
        ms = {"query": [], "all": [], "drifted": []}
        wall = []
        n_drifted = 0
        for _ in range(a.reps):
            b.repropagate(write=False)
            ms["query"].append(lib.vilo_last_repropagate_ms(ctx.h))
            r = b.repropagate(samples, offsets, point="given", lin=np.tile(base.lin, (W, 1)))   # back at the records' own point
            t0 = time.perf_counter()
            b.repropagate(samples, offsets)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms["all"].append(lib.vilo_last_repropagate_ms(ctx.h))
            b.repropagate(samples, offsets, point="given", lin=np.tile(base.lin, (W, 1)))
            r = b.repropagate(samples, offsets, select="drifted")
            ms["drifted"].append(lib.vilo_last_repropagate_ms(ctx.h))
            n_drifted = int(r.selected.sum())
        b.reset()
        after_ms = b.solve(opts)
        b.reset()
        b.set_samples()
        b.solve(opts)
        b.reset()
        samples_ms = b.solve(opts)
        print(json.dumps({"windows": W, "samples_per_window": n1, "repropagate_query_gpu_ms": round(min(ms["query"]), 4),
                          "repropagate_all_gpu_ms": round(min(ms["all"]), 3), "repropagate_all_wall_ms": round(min(wall), 2),
                          "repropagate_drifted_gpu_ms": round(min(ms["drifted"]), 3), "drifted_intervals": n_drifted, "intervals": 10 * W,
                          "solve_12_fixed_records_gpu_ms": round(fixed_ms, 3), "solve_12_after_repropagate_gpu_ms": round(after_ms, 3),
                          "solve_12_set_samples_gpu_ms": round(samples_ms, 3)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
