"""ms per vilo_batch_gyro_bias_align call (GPU time of k_gyro_bias_align, HIP events; both linearizations, with and without the
write-back, and with samples in force, where the call integrates every interval again on copies first) next to vilo_batch_residuals with
its optional outputs off and a 12-iteration solve of the same batch, at 128, 4096 and 32768 config-2 windows of 200 landmarks.
    python tools/time_gyro_align.py [--sizes 128,4096,32768] [--reps 5] > profiles/gyro_align_time.txt"""
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
        b.gyro_bias_align()   # (warm-up: the first call takes its arena chunks from the device)
        res_ms, rec_ms, cor_ms, write_ms, wall = [], [], [], [], []
        for _ in range(a.reps):
            b.residuals()
            res_ms.append(lib.vilo_last_residuals_ms(ctx.h))
            t0 = time.perf_counter()
            r = b.gyro_bias_align()
            wall.append(1e3 * (time.perf_counter() - t0))
            rec_ms.append(lib.vilo_last_gyro_align_ms(ctx.h))
            b.gyro_bias_align("corrected")
            cor_ms.append(lib.vilo_last_gyro_align_ms(ctx.h))
            b.gyro_bias_align("corrected", write=True)
            write_ms.append(lib.vilo_last_gyro_align_ms(ctx.h))
            b.reset()
        b.set_samples()
        b.gyro_bias_align()
        smp_ms = []
        for _ in range(a.reps):
            b.gyro_bias_align()
            smp_ms.append(lib.vilo_last_gyro_align_ms(ctx.h))
        g_ms = min(rec_ms)
        print(json.dumps({"windows": W, "intervals_per_window": int(r.n_intervals[0]), "status_ok": int((r.status == 0).sum()),
                          "max_abs_delta_bg": float(np.abs(r.delta_bg).max()), "solve12_gpu_ms": round(solve_ms, 3),
                          "residuals_gpu_ms": round(min(res_ms), 3), "gyro_gpu_ms": round(g_ms, 4), "gyro_corrected_gpu_ms": round(min(cor_ms), 4),
                          "gyro_write_gpu_ms": round(min(write_ms), 4), "gyro_samples_gpu_ms": round(min(smp_ms), 3),
                          "gyro_wall_ms": round(min(wall), 3), "ratio_to_residuals": round(g_ms / min(res_ms), 3),
                          "share_of_solve": round(g_ms / solve_ms, 5)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
