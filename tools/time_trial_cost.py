"""GPU ms per vilo_batch_trial_cost call (its four kernels, HIP events) at K = 1, 4 and 16 steps per window, next to K rounds of
vilo_batch_retract + vilo_batch_residuals on the same batch in the same process (what a caller paid per candidate before the call existed,
without the save / restore copies), at 128, 4096 and 32768 config-2 windows of 200 landmarks. Per size one JSON line: the minimum over
--reps calls of each, the time per step and the ratio of K rounds to the one call.
    python tools/time_trial_cost.py [--sizes 128,4096,32768] [--reps 5]"""
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
        step = {}
        for K in (1, 4, T.TRIAL_MAX_STEPS):
            s = np.ascontiguousarray(np.broadcast_to(1e-3 * rng.normal(size=(K, T.GRAD_STATE)), (W, K, T.GRAD_STATE)))
            lm = np.ascontiguousarray(np.broadcast_to(1e-3 * rng.normal(size=K * base.L), (W, K * base.L))).ravel()
            step[K] = (s, lm)
        r = b.trial_cost(*step[1])   # (warm-up)
        out["status_ok"] = int((r.status == 0).sum())
        b.save_state()
        ms = {k: [] for k in ("retract", "resid", 1, 4, T.TRIAL_MAX_STEPS)}
        for _ in range(a.reps):   # (interleaved: every call of a round sees the same clocks)
            b.retract(step[1][0][:, 0], step[1][1])
            ms["retract"].append(lib.vilo_last_retract_ms(ctx.h))
            b.residuals()
            ms["resid"].append(lib.vilo_last_residuals_ms(ctx.h))
            b.restore_state()
            for K in (1, 4, T.TRIAL_MAX_STEPS):
                b.trial_cost(*step[K], base=False, best=False)
                ms[K].append(lib.vilo_last_trial_cost_ms(ctx.h))
        rnd = min(ms["retract"]) + min(ms["resid"])
        out["retract_gpu_ms"], out["residuals_gpu_ms"], out["round_gpu_ms"] = round(min(ms["retract"]), 4), round(min(ms["resid"]), 4), round(rnd, 4)
        for K in (1, 4, T.TRIAL_MAX_STEPS):
            t = min(ms[K])
            out["trial_k%d_gpu_ms" % K] = round(t, 4)
            out["trial_k%d_per_step_ms" % K] = round(t / K, 4)
            out["k%d_rounds_over_trial" % K] = round(K * rnd / t, 3)
        out["spread_k1_max_over_min"] = round(max(ms[1]) / min(ms[1]), 3)
        print(json.dumps(out), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
