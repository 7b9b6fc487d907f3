"""Test helper: the definition of vilo_batch_triangulate (include/vilo_gpu.h, "landmark depths from the current poses") in numpy, in the
arrays the call returns: FeatureManager::triangulate's stereo and two-frame branches (feature_manager.cpp:302-382) with triangulatePoint's
null vector from numpy.linalg.svd, and removeBackShiftDepth's arithmetic (:450-479). Nothing of the kernel under test, nor of the host
library's Jacobi iteration."""
import numpy as np

SELECTED, STEREO, FALLBACK, NOT_FINITE = 1, 2, 4, 8

# FP64 floor of the definition in |d depth| / depth per branch, as tests/test_triangulate.py::test_fp64_floor_measured prints it (the
# largest of: every pose entry and observation moved by one unit in the last place; the compiled reference's FeatureManager; the host
# library's vilo_fw_triangulate — over that test's windows at the initial state and after a 4-iteration solve, rounded up; the
# solved states set it: there a few landmarks triangulate to more than a kilometre, rays all but parallel), and the GPU tolerances: ten times the floor.
# The shifted inverse depth is three matrix-vector products on the depth: it inherits the branch's figure.
FLOOR_STEREO, FLOOR_TWO_FRAME = 1e-11, 3e-11
TOL_STEREO, TOL_TWO_FRAME = 10 * FLOOR_STEREO, 10 * FLOOR_TWO_FRAME
FLOOR_SHIFT = 1e-15   # the back-shift of a GIVEN inverse depth (no triangulation before it), |d| / value: one unit in the last place, the reference
TOL_SHIFT = 10 * FLOOR_SHIFT


def quat_R(q):
    """rotation matrix of the normalised quaternion [x y z w] (Eigen's toRotationMatrix)"""
    x, y, z, w = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def poses(w):
    """(Ps [11, 3], Rs [11, 3, 3], tic [2, 3], ric [2, 3, 3]) of the window's state arrays; frames the window does not have: identity"""
    Ps, Rs = np.zeros((11, 3)), np.tile(np.eye(3), (11, 1, 1))
    for k in range(w.F):
        Ps[k], Rs[k] = w.pose[k, :3], quat_R(w.pose[k, 3:7])
    tic = np.array([w.ex_pose[c, :3] for c in range(2)])
    ric = np.array([quat_R(w.ex_pose[c, 3:7]) for c in range(2)])
    return Ps, Rs, tic, ric


def projection(Ps, Rs, tic, ric, k, cam):
    """[R0^T | -R0^T t0] of camera `cam` on frame k (feature_manager.cpp:312-325)"""
    t0 = Ps[k] + Rs[k] @ tic[cam]
    R0 = Rs[k] @ ric[cam]
    return np.hstack([R0.T, (-R0.T @ t0)[:, None]])


def triangulate_point(P0, P1, p0, p1):
    D = np.stack([p0[0] * P0[2] - P0[0], p0[1] * P0[2] - P0[1], p1[0] * P1[2] - P1[0], p1[1] * P1[2] - P1[1]])
    v = np.linalg.svd(D)[2][-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return v[:3] / v[3]


def window_triangulation(w, select="all", mask=None, write=False, init_depth=5.0, stereo=True):
    """dict of per-landmark arrays in the window's own order: depth, flags, shift_inv_depth, inv_depth (what the call leaves: changed
    only with write), z (localPoint.z() of a selected landmark, NaN elsewhere)"""
    Ps, Rs, tic, ric = poses(w)
    L = w.L
    depth, flags, z = np.zeros(L), np.zeros(L, np.uint8), np.full(L, np.nan)
    lam = w.inv_depth.copy()
    for l in range(L):
        o, s = w.lm_obs_offset[l], int(w.lm_start_frame[l])
        n_obs = w.lm_obs_offset[l + 1] - o
        st = bool(stereo) and bool(w.obs_is_stereo[o])
        sel = True if select == "all" else (bool(mask[l]) if select == "mask" else not (lam[l] > 0.0))
        if not st and n_obs < 2:
            sel = False
        with np.errstate(divide="ignore"):
            depth[l] = 1.0 / lam[l]
        if not sel:
            continue
        P0 = projection(Ps, Rs, tic, ric, s, 0)
        if st:
            P1, p1 = projection(Ps, Rs, tic, ric, s, 1), w.obs[o, 3:5]
        else:
            P1, p1 = projection(Ps, Rs, tic, ric, s + 1, 0), w.obs[o + 1, 0:2]
        X = triangulate_point(P0, P1, w.obs[o, 0:2], p1)
        z[l] = P0[2, :3] @ X + P0[2, 3]
        f = SELECTED | (STEREO if st else 0)
        if not np.isfinite(z[l]):
            f |= NOT_FINITE
        if z[l] > 0:
            depth[l] = z[l]
        else:
            depth[l], f = init_depth, f | FALLBACK
        flags[l] = f
        if write:
            lam[l] = 1.0 / depth[l]
    return dict(depth=depth, flags=flags, shift_inv_depth=back_shift(w, lam, init_depth), inv_depth=lam, z=z)


def back_shift(w, inv_depth, init_depth=5.0):
    """removeBackShiftDepth's arithmetic on the given inverse depths: landmarks of start frame 0 re-expressed in frame 1's left camera"""
    Ps, Rs, tic, ric = poses(w)
    mR, mP = Rs[0] @ ric[0], Ps[0] + Rs[0] @ tic[0]
    nR, nP = Rs[1] @ ric[0], Ps[1] + Rs[1] @ tic[0]
    out = np.array(inv_depth, float)
    for l in np.flatnonzero(w.lm_start_frame == 0):
        uv = w.obs[w.lm_obs_offset[l], 0:3]
        with np.errstate(divide="ignore"):
            pts_j = nR.T @ (mR @ (uv * (1.0 / inv_depth[l])) + mP - nP)
        out[l] = 1.0 / pts_j[2] if pts_j[2] > 0 else 1.0 / init_depth
    return out


def branch_errors(got_depth, ref):
    """(stereo, two-frame): max |d depth| / depth over the selected landmarks of each branch of `ref` (window_triangulation's dict)"""
    rel = np.abs(got_depth - ref["depth"]) / np.abs(ref["depth"])
    sel = (ref["flags"] & SELECTED) != 0
    st = sel & ((ref["flags"] & STEREO) != 0)
    tf = sel & ~st
    return (float(rel[st].max()) if st.any() else 0.0, float(rel[tf].max()) if tf.any() else 0.0)
