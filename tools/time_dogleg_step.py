"""GPU ms per vilo_batch_dogleg_step call (one linearisation + k_gn_step + k_dogleg, HIP events) next to the three calls a caller needed
before it — vilo_batch_gradient, vilo_batch_hessian_vector (K = 1) and vilo_batch_gauss_newton_step, each with a linearisation of its own
— on the same batch in the same process, at 128, 4096 and 32768 config-2 windows of 200 landmarks. Per size one JSON line: minimum and
median over --reps interleaved calls of each after a warm-up call, the spread (max / min), the three calls' sum, and k_dogleg alone
(vilo_set_profiling on its kernel kind, a second set of calls).
    python tools/time_dogleg_step.py [--sizes 128,4096,32768] [--reps 7]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,4096,32768")
    ap.add_argument("--reps", type=int, default=7)
    a = ap.parse_args()
    from cerberus_amd import api, synth
    from cerberus_amd import _ctypes as T
    cfg = synth.default_config()
    ctx = api.Context(cfg, 0)
    base = synth.make_window(cfg, params=synth.default_params(config=2, seed=20260925))
    ctx.preintegrate_window(base)
    lib = api.lib()
    lib.vilo_kernel_name.restype = C.c_char_p
    kind = [lib.vilo_kernel_name(i).decode() for i in range(32)].index("k_dogleg")
    rng = np.random.default_rng(1)
    for W in [int(s) for s in a.sizes.split(",")]:
        b = api.Batch(ctx, [base.twin() for _ in range(W)])
        out = {"windows": W, "landmarks": W * base.L}
        sv = np.ascontiguousarray(np.broadcast_to(rng.normal(size=T.GRAD_STATE), (W, T.GRAD_STATE)))
        lv = np.ascontiguousarray(np.broadcast_to(rng.normal(size=base.L), (W, base.L))).ravel()
        calls = {
            "gradient": (lambda: b.gradient(state=False, landmarks=False), lib.vilo_last_gradient_ms),
            "hess_vec_k1": (lambda: b.hessian_vector(sv, lv, state=False, landmarks=False), lib.vilo_last_hess_vec_ms),
            "gn_step": (lambda: b.gauss_newton_step(mu=1e-8, state=False, landmarks=False), lib.vilo_last_gn_step_ms),
            "dogleg_step": (lambda: b.dogleg_step(1e4, mu=1e-8), lib.vilo_last_dogleg_step_ms),
        }
        for f, _ in calls.values():   # (warm-up)
            r = f()
        out["status_ok"], out["branches"] = int((r.status == 0).sum()), np.bincount(r.branch[r.branch >= 0], minlength=3).tolist()
        ms = {k: [] for k in calls}
        for _ in range(a.reps):   # (interleaved: every call of a round sees the same clocks)
            for k, (f, last) in calls.items():
                f()
                ms[k].append(last(ctx.h))
        for k, v in ms.items():
            out[k + "_gpu_ms"] = {"min": round(min(v), 4), "median": round(float(np.median(v)), 4), "max_over_min": round(max(v) / min(v), 3)}
        three = [sum(ms[k][i] for k in ("gradient", "hess_vec_k1", "gn_step")) for i in range(a.reps)]
        out["three_calls_gpu_ms"] = {"min": round(min(three), 4), "median": round(float(np.median(three)), 4)}
        out["dogleg_over_three_calls"] = round(min(ms["dogleg_step"]) / min(three), 3)
        lib.vilo_set_profiling(ctx.h, 2 + kind)
        for _ in range(a.reps):
            b.dogleg_step(1e4, mu=1e-8)
        t, n = (C.c_double * 32)(), (C.c_longlong * 32)()
        lib.vilo_get_kernel_times(ctx.h, t, n, 32)
        lib.vilo_set_profiling(ctx.h, 0)
        out["k_dogleg_alone_gpu_ms_mean"] = round(t[kind] / max(1, n[kind]), 4)
        print(json.dumps(out), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
