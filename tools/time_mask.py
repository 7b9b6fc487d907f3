"""ms per vilo_batch_mask_landmarks call (GPU time of its kernels, HIP events) with a given mask and with the device's outlier test, next to
vilo_batch_residuals and a 12-iteration solve of the same batch (unmasked, masked and rebuilt without the masked landmarks), and next to
the alternative: vilo_batch_create of the reduced windows (host wall time), at 128, 4096 and 32768 config-2 windows of 200 landmarks.
    python tools/time_mask.py [--sizes 128,4096,32768] [--reps 5] [--share 0.05]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def without_landmarks(w, mask):
    """w's twin without the landmarks mask != 0: the window a caller would rebuild the batch from"""
    import copy
    keep = np.flatnonzero(np.asarray(mask) == 0)
    r = copy.copy(w.twin())
    idx = np.concatenate([np.arange(w.lm_obs_offset[l], w.lm_obs_offset[l + 1]) for l in keep]).astype(np.int64)
    r.obs, r.obs_is_stereo = np.ascontiguousarray(w.obs[idx]), np.ascontiguousarray(w.obs_is_stereo[idx])
    r.lm_obs_offset = np.concatenate([[0], np.cumsum(np.diff(w.lm_obs_offset)[keep])]).astype(np.int32)
    r.lm_start_frame, r.inv_depth = np.ascontiguousarray(w.lm_start_frame[keep]), np.ascontiguousarray(w.inv_depth[keep])
    r.truth_inv_depth = np.ascontiguousarray(w.truth_inv_depth[keep])
    r.L, r.n_obs = int(len(keep)), int(len(idx))
    return r


def timed_solve(b, opts, reps=3):
    """GPU ms of a solve from the uploaded state (reset before each: like for like between batches)"""
    out = []
    for _ in range(reps):
        b.reset()
        out.append(b.solve(opts))
    return min(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="128,4096,32768")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--share", type=float, default=0.05, help="share of the landmarks the given mask takes out")
    a = ap.parse_args()
    from cerberus_amd import api, synth
    cfg = synth.default_config()
    ctx = api.Context(cfg, 0)
    base = synth.make_window(cfg, params=synth.default_params(config=2, seed=20260925))
    ctx.preintegrate_window(base)
    lib = api.lib()
    one = (np.random.default_rng(1).random(base.L) < a.share).astype(np.uint8)
    reduced = without_landmarks(base, one)
    for W in [int(s) for s in a.sizes.split(",")]:
        b = api.Batch(ctx, [base.twin() for _ in range(W)])
        opts = api.default_solve_opts(True, 12)
        solve_ms = timed_solve(b, opts)
        b.residuals()
        resid_ms = min((b.residuals(), lib.vilo_last_residuals_ms(ctx.h))[1] for _ in range(a.reps))
        mask = np.tile(one, W)
        b.mask_landmarks(mask=mask)   # (warm-up: the first call allocates the second copy of the flag bytes)
        given_ms, outl_ms, given_wall = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter()
            b.mask_landmarks(mask=mask)
            given_wall.append(1e3 * (time.perf_counter() - t0))
            given_ms.append(lib.vilo_last_mask_ms(ctx.h))
            m, rec = b.mask_landmarks("outlier_flags")
            outl_ms.append(lib.vilo_last_mask_ms(ctx.h))
        b.mask_landmarks(mask=mask)
        b.reset()
        masked_solve_ms = timed_solve(b, opts)
        b.close()
        t0 = time.perf_counter()
        rb = api.Batch(ctx, [reduced.twin() for _ in range(W)])   # (the Python loop over the windows is part of neither figure)
        create_wall = 1e3 * (time.perf_counter() - t0)
        cm = (api.C.c_double * 4)()
        lib.vilo_last_create_ms(ctx.h, cm, None)
        rebuilt_solve_ms = timed_solve(rb, opts)
        rb.close()
        print(json.dumps({"windows": W, "landmarks": int(mask.size), "masked_given": int(mask.sum()), "masked_outlier_flags": int(m.sum()),
                          "mask_given_gpu_ms": round(min(given_ms), 4), "mask_given_wall_ms": round(min(given_wall), 3),
                          "mask_outlier_flags_gpu_ms": round(min(outl_ms), 4), "residuals_gpu_ms": round(resid_ms, 4),
                          "solve12_gpu_ms": round(solve_ms, 3), "solve12_masked_gpu_ms": round(masked_solve_ms, 3),
                          "solve12_rebuilt_gpu_ms": round(rebuilt_solve_ms, 3), "rebuild_create_ms": round(cm[0], 3),
                          "rebuild_create_with_python_wall_ms": round(create_wall, 3)}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
