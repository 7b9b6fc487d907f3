"""ms per vilo_batch_landmark_covariance call next to vilo_batch_covariance (GPU time of the linearisation + covariance kernels, HIP events;
and host wall time with the copies out) at 128, 4096 and 32768 config-2 windows of 200 landmarks.
    python tools/time_landmark_covariance.py [--sizes 128,4096,32768] [--reps 5]"""
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
        b.solve(api.default_solve_opts(True, 12))
        b.covariance()           # (warm-up: the first calls take their arena chunks from the device, later calls from the context's pool)
        b.landmark_covariance()
        cov_ms, lm_ms, lm_wall = [], [], []
        for _ in range(a.reps):
            b.covariance()
            cov_ms.append(lib.vilo_last_covariance_ms(ctx.h))
            t0 = time.perf_counter()
            r = b.landmark_covariance()
            lm_wall.append(1e3 * (time.perf_counter() - t0))
            lm_ms.append(lib.vilo_last_covariance_ms(ctx.h))
        c_ms, l_ms = min(cov_ms), min(lm_ms)
        print(json.dumps({"windows": W, "landmarks": int(r.offsets[-1]), "covariance_gpu_ms": round(c_ms, 3), "landmark_covariance_gpu_ms": round(l_ms, 3),
                          "landmark_covariance_wall_ms": round(min(lm_wall), 3), "ratio": round(l_ms / c_ms, 3), "status_ok": int((r.status == 0).sum())}),
              flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
