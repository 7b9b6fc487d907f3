"""ms per vilo_batch_residuals call (GPU time of its kernels, HIP events) with the optional outputs off and on, next to a 12-iteration solve
of the same batch, at 128, 4096 and 32768 config-2 windows of 200 landmarks.
    python tools/time_residuals.py [--sizes 128,4096,32768] [--reps 5]"""
import argparse
import json
import os
import sys
import time

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
        b.residuals(observations=True, imu=True)   # (warm-up: the first call uploads the observation rows and takes its arena chunks from the device)
        off_ms, on_ms, on_wall = [], [], []
        for _ in range(a.reps):
            r = b.residuals()
            off_ms.append(lib.vilo_last_residuals_ms(ctx.h))
            t0 = time.perf_counter()
            b.residuals(observations=True, imu=True)
            on_wall.append(1e3 * (time.perf_counter() - t0))
            on_ms.append(lib.vilo_last_residuals_ms(ctx.h))
        o_ms, n_ms = min(off_ms), min(on_ms)
        print(json.dumps({"windows": W, "landmarks": int(r.offsets[-1]), "solve12_gpu_ms": round(solve_ms, 3),
                          "residuals_gpu_ms": round(o_ms, 3), "residuals_all_outputs_gpu_ms": round(n_ms, 3),
                          "residuals_all_outputs_wall_ms": round(min(on_wall), 3), "share_of_solve": round(o_ms / solve_ms, 4),
                          "outliers": int(r.n_outliers.sum()), "status_ok": int((r.status == 0).sum())}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
