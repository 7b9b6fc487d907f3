"""Test helper: the definition of vilo_batch_predict_next_frame (include/vilo_gpu.h, "where the landmarks will be in the next frame's
cameras") in numpy, in the arrays the call returns, written from the header's text: the next pose (constant velocity or given), the
selection, pts_cam, pts_cam_right and the flags of one window. Nothing of the kernel under test."""
import collections

import numpy as np

import tri_ref

PREDICTED, BEHIND, NOT_FINITE, BEHIND_RIGHT = 1, 2, 4, 8
OK, TOO_FEW_FRAMES, NUMERIC = 0, 1, 2

# FP64 floor of the definition, as tests/test_predict.py::test_fp64_floor_measured prints it over every case of the GPU parity test: the
# largest of (a) every pose, extrinsic, first-observation point and inverse depth moved by one unit in the last place and (b) the 4 x 4
# homogeneous product curT inv(prevT) curT against the quaternion form. Metric: |d pts_cam|inf / max(1, |pts_cam|inf) per landmark; the
# pose: |d P|inf / max(1, |P|inf) and |d q|inf. Measured: points (a) 1.3e-15 (b) 6.0e-16, pose (a) 2.2e-16 (b) 1.1e-16; rounded up to one
# digit. The GPU tolerance is ten times the floor.
FLOOR = 2e-15
TOL = 10 * FLOOR

Prediction = collections.namedtuple("Prediction", "pts_cam pts_cam_right flags next_pose n_predicted status selected")


def quat_mul(a, b):
    """Hamilton product of [x y z w] quaternions"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def constant_velocity_pose(w):
    """[P_n, q_n] of nextT = curT (prevT^-1 curT), the header's quaternion form"""
    k = w.F - 1
    Ps, Rs, _, _ = tri_ref.poses(w)
    qk, qp = w.pose[k, 3:7] / np.linalg.norm(w.pose[k, 3:7]), w.pose[k - 1, 3:7] / np.linalg.norm(w.pose[k - 1, 3:7])
    q = quat_mul(qk, quat_mul(qp * np.array([-1.0, -1.0, -1.0, 1.0]), qk))
    return np.concatenate([Ps[k] + Rs[k] @ (Rs[k - 1].T @ (Ps[k] - Ps[k - 1])), q / np.linalg.norm(q)])


def constant_velocity_pose_4x4(w):
    """(P_n, R_n) the way the reference writes it: 4 x 4 homogeneous matrices, Matrix4d::inverse"""
    k = w.F - 1
    Ps, Rs, _, _ = tri_ref.poses(w)
    cur, prev = np.eye(4), np.eye(4)
    cur[:3, :3], cur[:3, 3] = Rs[k], Ps[k]
    prev[:3, :3], prev[:3, 3] = Rs[k - 1], Ps[k - 1]
    nxt = cur @ (np.linalg.inv(prev) @ cur)
    return nxt[:3, 3], nxt[:3, :3]


def selection(w):
    """the landmarks predicted (estimator.cpp:1708-1713)"""
    n_obs = np.diff(w.lm_obs_offset)
    return (w.inv_depth > 0) & (n_obs >= 2) & (w.lm_start_frame + n_obs - 1 == w.F - 1)


def points(w, Pn, Rn, cam=0, ric_transposed=False, tic_dropped=False):
    """pts_cam of every landmark of the window in camera `cam` of the next frame (P_n, R_n), selected or not (:1715-1719).
    ric_transposed / tic_dropped: the two mistakes tests/test_predict.py shows the skew-extrinsics window would catch."""
    Ps, Rs, tic, ric = tri_ref.poses(w)
    r0 = ric[0].T if ric_transposed else ric[0]
    t0 = np.zeros(3) if tic_dropped else tic[0]
    rc, tc = (r0, t0) if cam == 0 else (ric[1].T if ric_transposed else ric[1], np.zeros(3) if tic_dropped else tic[1])
    out = np.zeros((w.L, 3))
    for l in range(w.L):
        s = int(w.lm_start_frame[l])
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            pts_j = r0 @ (w.obs[w.lm_obs_offset[l], 0:3] * (1.0 / w.inv_depth[l])) + t0
            pts_w = Rs[s] @ pts_j + Ps[s]
            pts_local = Rn.T @ (pts_w - Pn)
            out[l] = rc.T @ (pts_local - tc)
    return out


def window_prediction(w, mode="constant_velocity", next_pose=None, right=False):
    """Prediction of one window at its state arrays: per-landmark arrays in the window's own order"""
    k = w.F - 1
    pts, ptr, flags = np.zeros((w.L, 3)), (np.zeros((w.L, 3)) if right else None), np.zeros(w.L, np.uint8)
    none = np.zeros(w.L, bool)
    if mode == "constant_velocity" and w.F < 3:
        return Prediction(pts, ptr, flags, w.pose[k].copy(), 0, TOO_FEW_FRAMES, none)
    used = [w.pose[:w.F], w.ex_pose if right else w.ex_pose[:1]]
    with np.errstate(invalid="ignore", divide="ignore"):
        if mode == "given":
            g = np.asarray(next_pose, float)
            pose = np.concatenate([g[:3], g[3:7] / np.linalg.norm(g[3:7])])
        else:
            pose = constant_velocity_pose(w)
    if not all(np.isfinite(a).all() for a in used + [pose]):
        return Prediction(pts, ptr, flags, w.pose[k].copy(), 0, NUMERIC, none)
    Pn, Rn = pose[:3], tri_ref.quat_R(pose[3:7])
    sel = selection(w)
    pts[sel] = points(w, Pn, Rn, 0)[sel]
    flags[sel] = PREDICTED
    with np.errstate(invalid="ignore"):
        flags[sel & ~(pts[:, 2] > 0)] |= BEHIND
        fin = np.isfinite(pts).all(axis=1)
        if right:
            ptr[sel] = points(w, Pn, Rn, 1)[sel]
            flags[sel & ~(ptr[:, 2] > 0)] |= BEHIND_RIGHT
            fin &= np.isfinite(ptr).all(axis=1)
    flags[sel & ~fin] |= NOT_FINITE
    return Prediction(pts, ptr, flags, pose, int(sel.sum()), OK, sel)


def point_error(got, ref):
    """max over the landmarks of |d pts|inf / max(1, |pts|inf)"""
    if not len(ref):
        return 0.0
    return float((np.abs(got - ref).max(axis=1) / np.maximum(1.0, np.abs(ref).max(axis=1))).max())


def pose_error(got, ref):
    """max(|d P|inf / max(1, |P|inf), |d q|inf)"""
    return float(max(np.abs(got[:3] - ref[:3]).max() / max(1.0, np.abs(ref[:3]).max()), np.abs(got[3:7] - ref[3:7]).max()))
