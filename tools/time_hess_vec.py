"""GPU ms per vilo_batch_hessian_vector call (linearisation + k_hess_vec, HIP events) at K = 1, 4 and 16 vectors per window, next to
vilo_batch_gradient (the same linearisation + k_gradient) and vilo_batch_gauss_newton_step on the same batch in the same process, at 128,
4096 and 32768 config-2 windows of 200 landmarks. Per size one JSON line: the minimum over --reps calls of each, the time per vector, the
kernel's share beyond the linearisation (call minus the gradient call, whose own kernel is 0.24 ms of it at 4096 windows: profiles/
gradient_time.txt) and K separate K = 1 calls for comparison.
    python tools/time_hess_vec.py [--sizes 128,4096,32768] [--reps 5]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,4096,32768")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from cerberus_amd import api, synth
    from cerberus_amd import _ctypes as T
    cfg = synth.default_config()
    ctx = api.Context(cfg, 0)
    base = synth.make_window(cfg, params=synth.default_params(config=2, seed=20260925))
    ctx.preintegrate_window(base)
    lib = api.lib()
    rng = np.random.default_rng(1)
    for W in [int(s) for s in a.sizes.split(",")]:
        b = api.Batch(ctx, [base.twin() for _ in range(W)])
        out = {"windows": W, "landmarks": W * base.L}
        vec = {}
        for K in (1, 4, T.HV_MAX_VECTORS):
            s = np.ascontiguousarray(np.broadcast_to(rng.normal(size=(K, T.GRAD_STATE)), (W, K, T.GRAD_STATE)))
            lm = np.ascontiguousarray(np.broadcast_to(rng.normal(size=K * base.L), (W, K * base.L))).ravel()
            vec[K] = (s, lm)
        r = b.hessian_vector(*vec[1], state=False, landmarks=False)   # (warm-up)
        out["status_ok"] = int((r.status == 0).sum())
        b.gauss_newton_step(mu=1e-8, state=False, landmarks=False)
        ms = {k: [] for k in ("grad", "step", 1, 4, T.HV_MAX_VECTORS)}
        for _ in range(a.reps):   # (interleaved: every call of a round sees the same clocks)
            b.gradient(state=False, landmarks=False)
            ms["grad"].append(lib.vilo_last_gradient_ms(ctx.h))
            b.gauss_newton_step(mu=1e-8, state=False, landmarks=False)
            ms["step"].append(lib.vilo_last_gn_step_ms(ctx.h))
            for K in (1, 4, T.HV_MAX_VECTORS):
                b.hessian_vector(*vec[K], state=False, landmarks=False)
                ms[K].append(lib.vilo_last_hess_vec_ms(ctx.h))
        grad = min(ms["grad"])
        out["gradient_gpu_ms"], out["gn_step_gpu_ms"] = round(grad, 4), round(min(ms["step"]), 4)
        for K in (1, 4, T.HV_MAX_VECTORS):
            t = min(ms[K])
            out["hess_vec_k%d_gpu_ms" % K] = round(t, 4)
            out["hess_vec_k%d_per_vector_ms" % K] = round(t / K, 4)
            out["hess_vec_k%d_beyond_gradient_call_ms" % K] = round(t - grad, 4)
            out["k%d_separate_k1_calls_ms" % K] = round(K * min(ms[1]), 4)
        out["spread_k1_max_over_min"] = round(max(ms[1]) / min(ms[1]), 3)
        print(json.dumps(out), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
