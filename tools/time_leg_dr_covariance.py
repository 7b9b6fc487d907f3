"""ms per vilo_batch_leg_dead_reckon_covariance call (GPU time of k_leg_dr_covariance, HIP events, after a warm-up, the minimum of 7
interleaved calls; with and without the two trajectories) next to vilo_batch_leg_dead_reckon and vilo_batch_dead_reckon_covariance on the
same batch and samples and vilo_preintegrate over the same intervals, from the same run, at 128, 4096 and 32768 config-2 windows with 30
samples each. The state is the one a solve leaves; cov_in is cut from the batch's own covariance at the smallest size and is a fixed
matrix at the others (vilo_batch_covariance of 32768 windows is not what is timed here). The host's packing and upload and the copies out
are outside the calls' GPU time; wall_ms is the whole Python call. vilo_preintegrate is a host-pointer call without an event timer of its
own: its figure is the wall time of the call, upload of the samples and download of the 15.6 KB records included, and is marked so.
    python tools/time_leg_dr_covariance.py [--sizes 128,4096,32768] [--samples 30] [--reps 7] > profiles/leg_dr_covariance_time.txt"""
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
    cin1 = None
    for W in [int(s) for s in a.sizes.split(",")]:
        b = api.Batch(ctx, [base.twin() for _ in range(W)])
        b.solve(api.default_solve_opts(True, 4))
        b.download()
        if cin1 is None:
            frames, _, _ = b.covariance(gauge="frame0")
            cin1 = api.leg_dr_cov_in(frames[:1], np.array([base.F]))[0]
        cin = np.ascontiguousarray(np.tile(cin1, (W, 1, 1)))
        cin15 = np.ascontiguousarray(cin[:, :15, :15])
        samples = np.ascontiguousarray(np.concatenate([base.samples[i % 64:i % 64 + a.samples] for i in range(W)]))
        offsets = np.arange(W + 1, dtype=np.int32) * a.samples
        f = base.F - 1
        lin = np.ascontiguousarray(np.tile(np.concatenate([base.speed_bias[f, 3:9], base.leg_bias[f]]), (W, 1)))
        r = b.leg_dead_reckon_covariance(samples, offsets, cin, pose_trajectory=True, leg_trajectory=True)   # (warm-up)
        b.leg_dead_reckon(samples, offsets)
        b.dead_reckon_covariance(samples, offsets, cin15)
        ctx.preintegrate(samples, offsets, lin)
        ms = {"cov": [], "traj": [], "leg": [], "imu_cov": [], "preint_wall": []}
        wall = []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            b.leg_dead_reckon_covariance(samples, offsets, cin)
            wall.append(1e3 * (time.perf_counter() - t0))
            ms["cov"].append(lib.vilo_last_leg_dr_cov_ms(ctx.h))
            b.leg_dead_reckon_covariance(samples, offsets, cin, pose_trajectory=True, leg_trajectory=True)
            ms["traj"].append(lib.vilo_last_leg_dr_cov_ms(ctx.h))
            b.leg_dead_reckon(samples, offsets)
            ms["leg"].append(lib.vilo_last_leg_dead_reckon_ms(ctx.h))
            b.dead_reckon_covariance(samples, offsets, cin15)
            ms["imu_cov"].append(lib.vilo_last_dr_cov_ms(ctx.h))
            t0 = time.perf_counter()
            ctx.preintegrate(samples, offsets, lin)
            ms["preint_wall"].append(1e3 * (time.perf_counter() - t0))
        c_ms = min(ms["cov"])
        print(json.dumps({"windows": W, "samples_per_window": a.samples, "steps": int(r.n_steps.sum()), "status_ok": int((r.status == 0).sum()),
                          "leg_dr_cov_gpu_ms": round(c_ms, 4), "leg_dr_cov_trajectories_gpu_ms": round(min(ms["traj"]), 4),
                          "leg_dead_reckon_gpu_ms": round(min(ms["leg"]), 4), "dead_reckon_covariance_gpu_ms": round(min(ms["imu_cov"]), 4),
                          "preintegrate_wall_ms": round(min(ms["preint_wall"]), 3), "leg_dr_cov_wall_ms": round(min(wall), 3),
                          "ns_per_step": round(1e6 * c_ms / max(1, int(r.n_steps.sum())), 3)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
