"""ms per vilo_batch_dead_reckon call (GPU time of k_dead_reckon, HIP events; with and without the trajectory) next to
vilo_batch_predict_next_frame on the same batch, at 128, 4096 and 32768 config-2 windows with 30 samples each. The state is the one a
solve leaves: where the call sits between two images. The host's packing and upload of the samples and the copies out are outside the
GPU time; wall_ms is the whole Python call.
    python tools/time_dead_reckon.py [--sizes 128,4096,32768] [--samples 30] [--reps 5] > profiles/dead_reckon_time.txt"""
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
        # window i reads a.samples rows of the generated stream from row i % 64 on: neighbouring lanes do not read the same bytes
        samples = np.ascontiguousarray(np.concatenate([base.samples[i % 64:i % 64 + a.samples] for i in range(W)]))
        offsets = np.arange(W + 1, dtype=np.int32) * a.samples
        r = b.dead_reckon(samples, offsets, trajectory=True)   # (warm-up: the first call takes its arena chunks from the device)
        b.predict_next_frame()
        ms = {"state": [], "trajectory": [], "predict": []}
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            b.dead_reckon(samples, offsets)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms["state"].append(lib.vilo_last_dead_reckon_ms(ctx.h))
            b.dead_reckon(samples, offsets, trajectory=True)
            ms["trajectory"].append(lib.vilo_last_dead_reckon_ms(ctx.h))
            b.predict_next_frame()
            ms["predict"].append(lib.vilo_last_predict_ms(ctx.h))
        s_ms = min(ms["state"])
        print(json.dumps({"windows": W, "samples_per_window": a.samples, "steps": int(r.n_steps.sum()), "status_ok": int((r.status == 0).sum()),
                          "dead_reckon_gpu_ms": round(s_ms, 4), "dead_reckon_trajectory_gpu_ms": round(min(ms["trajectory"]), 4),
                          "predict_gpu_ms": round(min(ms["predict"]), 4), "dead_reckon_wall_ms": round(min(wall), 3),
                          "ns_per_step": round(1e6 * s_ms / max(1, int(r.n_steps.sum())), 3),
                          "packed_bytes": int(56 * len(samples)), "ratio_to_predict": round(s_ms / min(ms["predict"]), 3)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
