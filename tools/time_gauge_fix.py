"""ms per vilo_batch_gauge_fix and vilo_batch_failure_detection call (GPU time of k_gauge_fix_x / k_failure_detection, HIP events) beside
the solve they follow, at 128, 4096 and 32768 config-2 windows, at the state a solve leaves. The anchor's and the last poses' uploads and
the copies out are outside the GPU time; wall_ms is the whole Python call. Reported, not gated.
    python tools/time_gauge_fix.py [--sizes 128,4096,32768] [--reps 5] > profiles/gauge_fix_time.txt"""
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
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from cerberus_amd import api, synth
    cfg = synth.default_config()
    ctx = api.Context(cfg, 0)
    base = synth.make_window(cfg, params=synth.default_params(config=2, seed=20260925))
    ctx.preintegrate_window(base)
    lib = api.lib()
    opts = api.default_solve_opts(True, 4)
    for W in [int(s) for s in a.sizes.split(",")]:
        ws = [base.twin() for _ in range(W)]
        b = api.Batch(ctx, ws)
        solve_ms = b.solve(opts)
        last = np.tile(base.pose[base.F - 2], (W, 1))
        tracks = np.full(W, 50, np.int32)
        g = b.gauge_fix()   # (warm-up: the first call takes its arena chunks from the device)
        f = b.failure_detection(tracks, last)
        ms = {"gauge": [], "given": [], "failure": []}
        wall = {"gauge": [], "failure": []}
        anchors = np.tile(base.pose[0], (W, 1))
        for _ in range(a.reps):
            b.reset()
            b.solve(opts)
            t0 = time.perf_counter()
            b.gauge_fix()
            wall["gauge"].append(1e3 * (time.perf_counter() - t0))
            ms["gauge"].append(lib.vilo_last_gauge_fix_ms(ctx.h))
            b.gauge_fix("given", anchors, pose0_before=True)
            ms["given"].append(lib.vilo_last_gauge_fix_ms(ctx.h))
            t0 = time.perf_counter()
            b.failure_detection(tracks, last)
            wall["failure"].append(1e3 * (time.perf_counter() - t0))
            ms["failure"].append(lib.vilo_last_failure_detection_ms(ctx.h))
        print(json.dumps({"windows": W, "gauge_ok": int((g.status == 0).sum()), "failure_ok": int((f.status == 0).sum()),
                          "solve_4_iterations_gpu_ms": round(solve_ms, 3), "gauge_fix_gpu_ms": round(min(ms["gauge"]), 4),
                          "gauge_fix_given_anchor_gpu_ms": round(min(ms["given"]), 4), "failure_detection_gpu_ms": round(min(ms["failure"]), 4),
                          "gauge_fix_wall_ms": round(min(wall["gauge"]), 3), "failure_detection_wall_ms": round(min(wall["failure"]), 3)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
