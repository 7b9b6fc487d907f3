"""ms per vilo_batch_dead_reckon_covariance call (GPU time of k_dr_covariance, HIP events; with and without the pose trajectory) next to
vilo_batch_dead_reckon and vilo_batch_covariance on the same batch, at 128, 4096 and 32768 config-2 windows with 30 samples each, cov_in
cut from the batch's own covariance. The state is the one a solve leaves: where the call sits between two images. The host's packing and
upload of the samples and of cov_in and the copies out are outside the GPU time; wall_ms is the whole Python call (minimum and median
over the repetitions).
    python tools/time_dr_covariance.py [--sizes 128,4096,32768] [--samples 30] [--reps 7] > profiles/dr_covariance_time.txt"""
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
    ap.add_argument("--reps", type=int, default=7)
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
        # window i reads a.samples rows of the generated stream from row i % 64 on: neighbouring windows do not read the same bytes
        samples = np.ascontiguousarray(np.concatenate([base.samples[i % 64:i % 64 + a.samples] for i in range(W)]))
        offsets = np.arange(W + 1, dtype=np.int32) * a.samples
        frames, _, cst = b.covariance()   # (warm-up of the covariance call as well)
        cov_in = api.dr_cov_in(frames, np.full(W, base.F))
        r = b.dead_reckon_covariance(samples, offsets, cov_in, pose_trajectory=True)   # (warm-up: the first call takes its arena chunks from the device)
        b.dead_reckon(samples, offsets)
        ms = {"cov": [], "trajectory": [], "null": [], "dead_reckon": [], "covariance": []}
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            b.dead_reckon_covariance(samples, offsets, cov_in)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms["cov"].append(lib.vilo_last_dr_cov_ms(ctx.h))
            b.dead_reckon_covariance(samples, offsets, cov_in, pose_trajectory=True)
            ms["trajectory"].append(lib.vilo_last_dr_cov_ms(ctx.h))
            b.dead_reckon_covariance(samples, offsets)
            ms["null"].append(lib.vilo_last_dr_cov_ms(ctx.h))
            b.dead_reckon(samples, offsets)
            ms["dead_reckon"].append(lib.vilo_last_dead_reckon_ms(ctx.h))
            b.covariance()
            ms["covariance"].append(lib.vilo_last_covariance_ms(ctx.h))
        c_ms = min(ms["cov"])
        steps = int(r.n_steps.sum())
        print(json.dumps({"windows": W, "samples_per_window": a.samples, "steps": steps, "status_ok": int((r.status == 0).sum()),
                          "covariance_status_ok": int((cst == 0).sum()),
                          "dr_cov_gpu_ms": round(c_ms, 4), "dr_cov_gpu_ms_median": round(float(np.median(ms["cov"])), 4),
                          "dr_cov_trajectory_gpu_ms": round(min(ms["trajectory"]), 4), "dr_cov_null_cov_in_gpu_ms": round(min(ms["null"]), 4),
                          "dead_reckon_gpu_ms": round(min(ms["dead_reckon"]), 4), "batch_covariance_gpu_ms": round(min(ms["covariance"]), 4),
                          "dr_cov_wall_ms": round(min(wall), 3), "dr_cov_wall_ms_median": round(float(np.median(wall)), 3),
                          "ns_per_step": round(1e6 * c_ms / max(1, steps), 3),
                          "ratio_to_dead_reckon": round(c_ms / min(ms["dead_reckon"]), 2)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
