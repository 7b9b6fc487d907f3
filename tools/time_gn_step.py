"""GPU ms per vilo_batch_gauss_newton_step call (linearisation + k_gn_step, HIP events) in both kernel forms (the coupling streamed through
global memory, two workgroups per CU; resident in LDS, one) next to vilo_batch_gradient, vilo_batch_covariance
and a 12-iteration solve of the same batch, at 128, 4096 and 32768 config-2 windows of 200 landmarks.
    python tools/time_gn_step.py [--sizes 128,4096,32768] [--reps 5]"""
import argparse
import json
import os
import sys

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
        for _ in range(3):
            b.reset()
            solve_ms.append(b.solve(opts))
        b.reset()
        step, step0, grad, cov, res = [], [], [], [], []
        r = b.gauss_newton_step(mu=1e-8, state=False, landmarks=False)   # (warm-up)
        for _ in range(a.reps):
            b.gauss_newton_step(mu=1e-8, state=False, landmarks=False)
            step.append(lib.vilo_last_gn_step_ms(ctx.h))
            b.gauss_newton_step(mu=0.0, gauge="frame0", state=False, landmarks=False)
            step0.append(lib.vilo_last_gn_step_ms(ctx.h))
            ctx.set_gn_step_form("resident")
            b.gauss_newton_step(mu=1e-8, state=False, landmarks=False)
            res.append(lib.vilo_last_gn_step_ms(ctx.h))
            ctx.set_gn_step_form("streamed")
            b.gradient(state=False, landmarks=False)
            grad.append(lib.vilo_last_gradient_ms(ctx.h))
            b.covariance()
            cov.append(lib.vilo_last_covariance_ms(ctx.h))
        print(json.dumps({"windows": W, "landmarks": W * base.L, "status_ok": int((r.status == 0).sum()),
                          "gn_step_gpu_ms": round(min(step), 4), "gn_step_frame0_gpu_ms": round(min(step0), 4), "gn_step_resident_form_gpu_ms": round(min(res[1:] or res), 4),
                          "gradient_gpu_ms": round(min(grad), 4), "covariance_gpu_ms": round(min(cov), 4),
                          "solve12_gpu_ms": round(min(solve_ms), 3)}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
