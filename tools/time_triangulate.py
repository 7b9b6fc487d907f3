"""ms per vilo_batch_triangulate call (GPU time of k_triangulate, HIP events; every landmark selected, with and without the write-back and
the shifted depths) next to vilo_batch_residuals with its optional outputs off (the nearest neighbour: one walk over the same packed
waves) and a 12-iteration solve of the same batch, at 128, 4096 and 32768 config-2 windows of 200 landmarks. For information, the host
library's FeatureWindow::triangulate over one window's landmarks on one core, times the number of windows.
    python tools/time_triangulate.py [--sizes 128,4096,32768] [--reps 5] > profiles/triangulate_time.txt"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def quat_R(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def host_triangulate_ms(w, reps=20):
    """one window's tracks through the host feature window; ms per triangulate() of all of them (clearDepth before each)"""
    path = os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_host.so")
    if not os.path.exists(path):
        return None
    lib = C.CDLL(path)
    lib.vilo_fw_create.restype = C.c_void_p
    h = C.c_void_p(lib.vilo_fw_create())
    dp, ip, up = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_ubyte)
    n_obs = np.diff(w.lm_obs_offset)
    for fc in range(w.F):
        ids = np.flatnonzero((w.lm_start_frame <= fc) & (fc < w.lm_start_frame + n_obs)).astype(np.int32)
        rows = w.lm_obs_offset[ids] + fc - w.lm_start_frame[ids]
        obs, st = np.ascontiguousarray(w.obs[rows]), np.ascontiguousarray(w.obs_is_stereo[rows])
        lib.vilo_fw_add_frame(h, C.c_int(fc), C.c_int(len(ids)), ids.ctypes.data_as(ip), obs.ctypes.data_as(dp), st.ctypes.data_as(up),
                              C.c_double(float(w.td[0])), None)
    Ps = np.ascontiguousarray(w.pose[:, :3])
    Rs = np.ascontiguousarray(np.stack([quat_R(w.pose[k, 3:7]) for k in range(w.F)]))
    tic = np.ascontiguousarray(w.ex_pose[:, :3])
    ric = np.ascontiguousarray(np.stack([quat_R(w.ex_pose[c, 3:7]) for c in range(2)]))
    args = [x.ctypes.data_as(dp) for x in (Ps, Rs, tic, ric)]
    best = 1e30
    for _ in range(reps):
        lib.vilo_fw_clear_depth(h)
        t0 = time.perf_counter()
        lib.vilo_fw_triangulate(h, *args)
        best = min(best, 1e3 * (time.perf_counter() - t0))
    lib.vilo_fw_destroy(h)
    return best


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
    host_ms = host_triangulate_ms(base)
    lib = api.lib()
    for W in [int(s) for s in a.sizes.split(",")]:
        b = api.Batch(ctx, [base.twin() for _ in range(W)])
        opts = api.default_solve_opts(True, 12)
        solve_ms = min(b.solve(opts) for _ in range(2))
        b.residuals()
        b.triangulate("all", shift=True)   # (warm-up: the first call takes its arena chunks from the device)
        res_ms, tri_ms, two_ms, full_ms, wall = [], [], [], [], []
        for _ in range(a.reps):
            b.residuals()
            res_ms.append(lib.vilo_last_residuals_ms(ctx.h))
            t0 = time.perf_counter()
            r = b.triangulate("all")
            wall.append(1e3 * (time.perf_counter() - t0))
            tri_ms.append(lib.vilo_last_triangulate_ms(ctx.h))
            b.triangulate("all", stereo=False)
            two_ms.append(lib.vilo_last_triangulate_ms(ctx.h))
            b.reset()
            b.triangulate("all", write=True, shift=True)
            full_ms.append(lib.vilo_last_triangulate_ms(ctx.h))
        t_ms, r_ms = min(tri_ms), min(res_ms)
        print(json.dumps({"windows": W, "landmarks": int(r.offsets[-1]), "solve12_gpu_ms": round(solve_ms, 3), "residuals_gpu_ms": round(r_ms, 3),
                          "triangulate_gpu_ms": round(t_ms, 3), "triangulate_two_frame_gpu_ms": round(min(two_ms), 3),
                          "triangulate_write_shift_gpu_ms": round(min(full_ms), 3), "triangulate_wall_ms": round(min(wall), 3),
                          "ratio_to_residuals": round(t_ms / r_ms, 3), "share_of_solve": round(t_ms / solve_ms, 5),
                          "host_feature_window_one_core_ms": None if host_ms is None else round(host_ms * W, 1),
                          "fallbacks": int(((r.flags & 4) != 0).sum()), "not_finite": int(((r.flags & 8) != 0).sum())}), flush=True)
        b.close()
    ctx.close()


if __name__ == "__main__":
    main()
