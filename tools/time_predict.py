"""ms per vilo_batch_predict_next_frame call (GPU time of k_predict_next_frame + k_predict_windows, HIP events; both modes, with and
without the right camera) next to vilo_batch_residuals with its optional outputs off and a 12-iteration solve of the same batch, at 128,
4096 and 32768 config-2 windows of 200 landmarks. The state is the one the solve leaves: where the call sits in processImage.
    python tools/time_predict.py [--sizes 128,4096,32768] [--reps 5] > profiles/predict_time.txt"""
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
        b.residuals()
        r = b.predict_next_frame(right=True)   # (warm-up: the first call takes its arena chunks from the device)
        pose = r.next_pose
        res_ms, wall = [], []
        ms = {"cv": [], "cv_right": [], "given": [], "given_right": []}
        for _ in range(a.reps):
            b.residuals()
            res_ms.append(lib.vilo_last_residuals_ms(ctx.h))
            t0 = time.perf_counter()
            b.predict_next_frame()
            wall.append(1e3 * (time.perf_counter() - t0))
            ms["cv"].append(lib.vilo_last_predict_ms(ctx.h))
            b.predict_next_frame(right=True)
            ms["cv_right"].append(lib.vilo_last_predict_ms(ctx.h))
            b.predict_next_frame("given", pose)
            ms["given"].append(lib.vilo_last_predict_ms(ctx.h))
            b.predict_next_frame("given", pose, right=True)
            ms["given_right"].append(lib.vilo_last_predict_ms(ctx.h))
        p_ms = min(ms["cv"])
        print(json.dumps({"windows": W, "landmarks": int(r.offsets[-1]), "predicted": int(r.n_predicted.sum()), "status_ok": int((r.status == 0).sum()),
                          "solve12_gpu_ms": round(solve_ms, 3), "residuals_gpu_ms": round(min(res_ms), 3), "predict_gpu_ms": round(p_ms, 4),
                          "predict_right_gpu_ms": round(min(ms["cv_right"]), 4), "predict_given_gpu_ms": round(min(ms["given"]), 4),
                          "predict_given_right_gpu_ms": round(min(ms["given_right"]), 4), "predict_wall_ms": round(min(wall), 3),
                          "ratio_to_residuals": round(p_ms / min(res_ms), 3), "share_of_solve": round(p_ms / solve_ms, 5)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
