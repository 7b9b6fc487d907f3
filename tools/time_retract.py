"""ms per vilo_batch_retract call (GPU time of k_retract, HIP events; and host wall time with the steps' upload and the records' download)
with a full step and with NULL steps, next to vilo_batch_reset (a device copy of the same state bytes; host wall time up to the stream's
drain, which a small vilo_debug_fetch forces, less that fetch alone), vilo_batch_save_state / _restore_state (the same way) and a
12-iteration solve, at 128, 4096 and 32768 config-2 windows of 200 landmarks.
    python tools/time_retract.py [--sizes 128,4096,32768] [--reps 5]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def wall_ms(fn, reps):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append(1e3 * (time.perf_counter() - t0))
    return min(out)


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
    rng = np.random.default_rng(1)
    for W in [int(s) for s in a.sizes.split(",")]:
        b = api.Batch(ctx, [base.twin() for _ in range(W)])
        opts = api.default_solve_opts(True, 12)
        solve_ms = []
        for _ in range(3):
            b.reset()
            solve_ms.append(b.solve(opts))
        ss, ls, alpha = 1e-3 * rng.normal(size=(W, 222)), 1e-3 * rng.normal(size=W * base.L), 0.5 + rng.random(W)
        b.retract(ss, ls, alpha, base="uploaded")   # (warm-up)
        full_gpu, full_wall, null_gpu = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            r = b.retract(ss, ls, alpha, base="uploaded")
            full_wall.append(1e3 * (time.perf_counter() - t0))
            full_gpu.append(lib.vilo_last_retract_ms(ctx.h))
            b.retract(base="uploaded")
            null_gpu.append(lib.vilo_last_retract_ms(ctx.h))
        drain = lambda: b.fetch(10, 0, max_n=128)
        drain_ms = wall_ms(drain, a.reps)
        b.save_state()
        drain()
        reset_ms = wall_ms(lambda: (b.reset(), drain()), a.reps) - drain_ms
        save_ms = wall_ms(lambda: (b.save_state(), drain()), a.reps) - drain_ms
        restore_ms = wall_ms(lambda: (b.restore_state(), drain()), a.reps) - drain_ms
        print(json.dumps({"windows": W, "landmarks": W * base.L, "applied_per_window": int(r.n_applied[0]),
                          "retract_gpu_ms": round(min(full_gpu), 4), "retract_wall_ms": round(min(full_wall), 3),
                          "retract_null_steps_gpu_ms": round(min(null_gpu), 4), "reset_wall_ms": round(reset_ms, 4),
                          "save_state_wall_ms": round(save_ms, 4), "restore_state_wall_ms": round(restore_ms, 4),
                          "solve12_gpu_ms": round(min(solve_ms), 3)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
