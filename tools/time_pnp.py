"""ms per vilo_batch_frame_pose_pnp call (GPU time of k_frame_pose_pnp, HIP events; the windows' last frame from the previous frame's
pose, default options, with and without the write-back) next to vilo_batch_triangulate over every landmark, vilo_batch_residuals with its
optional outputs off and a 12-iteration solve of the same batch, at 128, 4096 and 32768 config-2 windows of 200 landmarks.
    python tools/time_pnp.py [--sizes 128,4096,32768] [--reps 5] > profiles/pnp_time.txt"""
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
    for W in [int(s) for s in a.sizes.split(",")]:
        b = api.Batch(ctx, [base.twin() for _ in range(W)])
        opts = api.default_solve_opts(True, 12)
        solve_ms = min(b.solve(opts) for _ in range(2))
        b.reset()
        b.residuals()
        b.triangulate("all")
        b.frame_pose_pnp()   # (warm-up: the first call takes its arena chunks from the device)
        res_ms, tri_ms, pnp_ms, write_ms, wall = [], [], [], [], []
        for _ in range(a.reps):
            b.residuals()
            res_ms.append(lib.vilo_last_residuals_ms(ctx.h))
            b.triangulate("all")
            tri_ms.append(lib.vilo_last_triangulate_ms(ctx.h))
            t0 = time.perf_counter()
            r = b.frame_pose_pnp()
            wall.append(1e3 * (time.perf_counter() - t0))
            pnp_ms.append(lib.vilo_last_pnp_ms(ctx.h))
            b.frame_pose_pnp(write=True)
            write_ms.append(lib.vilo_last_pnp_ms(ctx.h))
            b.reset()
        p_ms = min(pnp_ms)
        print(json.dumps({"windows": W, "points_per_window": int(r.n_points[0]), "steps": int(r.iterations.max()),
                          "status_ok": int((r.status == 0).sum()), "solve12_gpu_ms": round(solve_ms, 3),
                          "residuals_gpu_ms": round(min(res_ms), 3), "triangulate_gpu_ms": round(min(tri_ms), 3), "pnp_gpu_ms": round(p_ms, 3),
                          "pnp_write_gpu_ms": round(min(write_ms), 3), "pnp_wall_ms": round(min(wall), 3),
                          "ratio_to_residuals": round(p_ms / min(res_ms), 3), "share_of_solve": round(p_ms / solve_ms, 5)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
