"""ms per vilo_batch_gradient call (GPU time: the mode-0 linearisation + k_gradient, HIP events) next to vilo_batch_covariance's time and a
12-iteration solve of the same batch, at 128, 4096 and 32768 config-2 windows of 200 landmarks. The linearisation's own share comes from a
kernel trace of this script (k_gradient's row against the linearisation kernels').
    python tools/time_gradient.py [--sizes 128,4096,32768] [--reps 5] > profiles/gradient_time.txt"""
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
        b.gradient()   # (warm-up: the first call takes its arena chunks from the device)
        rec_ms, all_ms, all_wall = [], [], []
        for _ in range(a.reps):
            r = b.gradient(state=False, landmarks=False)
            rec_ms.append(lib.vilo_last_gradient_ms(ctx.h))
            t0 = time.perf_counter()
            b.gradient()
            all_wall.append(1e3 * (time.perf_counter() - t0))
            all_ms.append(lib.vilo_last_gradient_ms(ctx.h))
        g_ms = min(min(rec_ms), min(all_ms))
        print(json.dumps({"windows": W, "landmarks": int(r.offsets[-1]), "solve12_gpu_ms": round(solve_ms, 3), "gradient_gpu_ms": round(g_ms, 3),
                          "gradient_all_outputs_wall_ms": round(min(all_wall), 3), "share_of_solve": round(g_ms / solve_ms, 4),
                          "max_scaled_max": float(r.scaled_max.max()), "status_ok": int((r.status == 0).sum())}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
