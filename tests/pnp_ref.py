"""Test helper: the definition of vilo_batch_frame_pose_pnp (include/vilo_gpu.h, "frame pose by PnP") in numpy: the selection rule of
FeatureManager::initFramePoseByPnP (feature_manager.cpp:259-300) without the landmarks that start on the frame, and plain Gauss-Newton on
the reprojection error with a left-multiplicative perturbation of cam_T_w, the step from numpy.linalg.solve. A second, independently
parameterised minimiser (right-multiplicative perturbation of w_T_cam, numpy.linalg.lstsq on the stacked Jacobian) measures the floor.
Nothing of the kernel under test."""
import collections

import numpy as np

from tri_ref import poses, quat_R

OK, NOT_ENOUGH_POINTS, NO_CONVERGENCE, NUMERIC, NO_FRAME = 0, 1, 2, 3, 4

# FP64 floor of the definition, as tests/test_pnp.py::test_fp64_floor_measured prints it: the larger of (a) the minimiser's movement when
# every pose entry, inverse depth and observation it reads moves by one unit in the last place and (b) `frame_pose` against
# `frame_pose_right` — position |dP| / max(1, |P|), rotation the angle of Ra^T Rb — over that test's cases (the four packing shapes at the
# initial state and after a 4-iteration solve, last frame and frame 2), rounded up to one significant digit; the GPU tolerances are ten
# times the floor. Measured: position (a) 2.3e-15 (b) 2.3e-15, rotation (a) 4.9e-16 (b) 3.3e-16 — the problems are well
# conditioned (cond(J^T J) about 1e2, every point more than 1.7 m in front of the camera), so the floor is a few units in the last place.
FLOOR_POS, FLOOR_ROT = 3e-15, 5e-16
TOL_POS, TOL_ROT = 10 * FLOOR_POS, 10 * FLOOR_ROT
# step_tolerance of the GPU parity calls: Gauss-Newton converges linearly on these problems, and the default stop (1e-12) leaves up to 2e-14
# of truncation error, more than the rotation tolerance; at 1e-14 the stop leaves less than the floor (tests/test_pnp.py prints both)
PARITY_STEP_TOLERANCE = 1e-14
TOL_COST = 1e-10          # final_cost relative to the reference's
STATIONARY = 1e-12        # |J^T r|_inf <= STATIONARY * max(1, |J^T J|_inf) at the reference's result

Result = collections.namedtuple("Result", "pose final_cost initial_cost n_points iterations status R P H g")


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def exp_so3(w):
    th = np.linalg.norm(w)
    K = skew(w)
    if th < 1e-4:
        a, b = 1.0 - th * th / 6.0, 0.5 - th * th / 24.0
    else:
        a, b = np.sin(th) / th, (1.0 - np.cos(th)) / (th * th)
    return np.eye(3) + a * K + b * (K @ K)


def quat_of(R):
    """[x y z w] of a rotation matrix, normalised, w >= 0"""
    w = np.sqrt(max(0.0, 1.0 + R[0, 0] + R[1, 1] + R[2, 2])) / 2.0
    if w > 0.25:
        q = np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q = np.zeros(4)
        q[i], q[j], q[k], q[3] = 0.5 * s, (R[j, i] + R[i, j]) / (2 * s), (R[k, i] + R[i, k]) / (2 * s), (R[k, j] - R[j, k]) / (2 * s)
    q /= np.linalg.norm(q)
    return -q if q[3] < 0 else q


def frame_of(w, frame):
    return w.F - 1 if frame < 0 else frame


def points(w, k):
    """(X [n, 3] world points, uv [n, 2] image points on frame k, ids [n] landmark indices) of the landmarks the definition uses"""
    Ps, Rs, tic, ric = poses(w)
    X, uv, ids = [], [], []
    for l in range(w.L):
        o, s = w.lm_obs_offset[l], int(w.lm_start_frame[l])
        n_obs = w.lm_obs_offset[l + 1] - o
        if not (w.inv_depth[l] > 0.0) or not (1 <= k - s < n_obs):
            continue
        X.append(Rs[s] @ (ric[0] @ (w.obs[o, 0:3] / w.inv_depth[l]) + tic[0]) + Ps[s])
        uv.append(w.obs[o + k - s, 0:2])
        ids.append(l)
    return np.array(X).reshape(-1, 3), np.array(uv).reshape(-1, 2), np.array(ids, int)


def start(w, k, guess):
    """(RCam, PCam): w_T_cam of the left camera on frame k - 1 ('previous') or k ('current')"""
    Ps, Rs, tic, ric = poses(w)
    g = k if guess == "current" else k - 1
    return Rs[g] @ ric[0], Rs[g] @ tic[0] + Ps[g]


def linearize(R, t, X, uv):
    """(J [2n, 6], r [2n], min z) at cam_T_w = (R, t), columns (dtheta, dt) of the left-multiplicative perturbation"""
    Y = X @ R.T + t
    z = Y[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        r = (Y[:, :2] / z[:, None] - uv).reshape(-1)
        J = np.zeros((2 * len(X), 6))
        for i, y in enumerate(Y):
            Jp = np.array([[1.0 / y[2], 0.0, -y[0] / y[2] ** 2], [0.0, 1.0 / y[2], -y[1] / y[2] ** 2]])
            J[2 * i:2 * i + 2] = Jp @ np.hstack([-skew(y), np.eye(3)])
    return J, r, (z.min() if len(z) else np.inf)


def body_pose(w, RCam, PCam):
    _, _, tic, ric = poses(w)
    Rk = RCam @ ric[0].T
    Pk = -Rk @ tic[0] + PCam
    return np.concatenate([Pk, quat_of(Rk)]), Rk, Pk


def frame_pose(w, frame=-1, guess="previous", max_iterations=100, step_tolerance=1e-13):
    """The definition. The defaults iterate until |delta| < 1e-13 (the converged reference); with the call's own max_iterations and
    step_tolerance it returns the status and step count the call must report."""
    k = frame_of(w, frame)
    cur = np.array(w.pose[k], float) if k < w.F else np.array([0, 0, 0, 0, 0, 0, 1.0])
    if not 1 <= k <= w.F - 1:
        return Result(cur, 0.0, 0.0, 0, 0, NO_FRAME, None, None, None, None)
    X, uv, _ = points(w, k)
    n = len(X)
    if n < 4:
        return Result(cur, 0.0, 0.0, n, 0, NOT_ENOUGH_POINTS, None, None, None, None)
    RCam, PCam = start(w, k, guess)
    R = RCam.T
    t = -R @ PCam
    it, converged, c0 = 0, False, None
    while True:
        J, r, zmin = linearize(R, t, X, uv)
        cost = 0.5 * float(r @ r)
        c0 = cost if c0 is None else c0
        H, g = J.T @ J, J.T @ r
        if not (zmin > 0.0) or not np.isfinite(cost):
            return Result(cur, cost, c0, n, it, NUMERIC, None, None, H, g)
        if converged or it == max_iterations:
            break
        try:
            np.linalg.cholesky(H)
        except np.linalg.LinAlgError:
            return Result(cur, cost, c0, n, it, NUMERIC, None, None, H, g)
        d = np.linalg.solve(H, -g)
        E = exp_so3(d[:3])
        R, t = E @ R, E @ t + d[3:]
        it += 1
        converged = np.linalg.norm(d) <= step_tolerance
    pose, Rk, Pk = body_pose(w, R.T, -R.T @ t)
    return Result(pose, cost, c0, n, it, OK if converged else NO_CONVERGENCE, Rk, Pk, H, g)


def frame_pose_right(w, frame=-1, guess="previous", max_iterations=100, step_tolerance=1e-13):
    """The same minimiser parameterised the other way: w_T_cam = (Rw, Pw) with the right-multiplicative perturbation Rw <- Rw Exp(a),
    Pw <- Pw + Rw b, the step from numpy.linalg.lstsq on the stacked Jacobian. Returns (Rk, Pk) of the body."""
    k = frame_of(w, frame)
    X, uv, _ = points(w, k)
    Rw, Pw = start(w, k, guess)
    for _ in range(max_iterations):
        Y = (X - Pw) @ Rw   # rows Rw^T (X - Pw)
        r = (Y[:, :2] / Y[:, 2:3] - uv).reshape(-1)
        J = np.zeros((2 * len(X), 6))
        for i, y in enumerate(Y):
            Jp = np.array([[1.0 / y[2], 0.0, -y[0] / y[2] ** 2], [0.0, 1.0 / y[2], -y[1] / y[2] ** 2]])
            J[2 * i:2 * i + 2] = Jp @ np.hstack([skew(y), -np.eye(3)])   # Y' = Exp(-a) (Y - b)
        d = np.linalg.lstsq(J, -r, rcond=None)[0]
        Rw, Pw = Rw @ exp_so3(d[:3]), Pw + Rw @ d[3:]
        if np.linalg.norm(d) < step_tolerance:
            break
    _, Rk, Pk = body_pose(w, Rw, Pw)
    return Rk, Pk


def pose_errors(pose, Rk, Pk):
    """(position, rotation) error of a pose row [p, q] against the body pose (Rk, Pk): |dP| / max(1, |P|), the angle of Ra^T Rb"""
    return rigid_errors(quat_R(pose[3:7]), np.asarray(pose[:3]), Rk, Pk)


def rigid_errors(Ra, Pa, Rb, Pb):
    dR = Ra.T @ Rb
    s = np.linalg.norm([dR[2, 1] - dR[1, 2], dR[0, 2] - dR[2, 0], dR[1, 0] - dR[0, 1]]) / 2.0   # sin(angle): exact for tiny angles
    ang = float(np.arctan2(s, (np.trace(dR) - 1.0) / 2.0))
    return float(np.linalg.norm(Pa - Pb) / max(1.0, np.linalg.norm(Pb))), ang
