"""ms per vilo_batch_covariance call (GPU time of the linearisation + covariance kernels, HIP events; and host wall time with the copy of
the frame blocks out) at 128, 4096 and 32768 config-2 windows, next to one 12-iteration vilo_batch_solve of the same batch.
    python tools/time_covariance.py [--sizes 128,4096,32768] [--reps 5]"""
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
        solve_ms = []
        for _ in range(a.reps):
            b.reset()
            solve_ms.append(b.solve(opts))
        b.covariance()   # (warm-up: the first call takes its arena chunks from the device, later calls from the context's pool)
        cov_ms, wall_ms = [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            _, _, st = b.covariance()
            wall_ms.append(1e3 * (time.perf_counter() - t0))
            cov_ms.append(lib.vilo_last_covariance_ms(ctx.h))
        s_ms, c_ms = min(solve_ms), min(cov_ms)
        print(json.dumps({"windows": W, "solve_ms": round(s_ms, 3), "covariance_gpu_ms": round(c_ms, 3), "covariance_wall_ms": round(min(wall_ms), 3),
                          "ratio_to_solve": round(c_ms / s_ms, 3), "status_ok": int((st == 0).sum())}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
