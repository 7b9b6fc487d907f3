"""Test helper: the definitions of vilo_batch_residuals (include/vilo_gpu.h) restated with numpy on the oracle's factor evaluations. Every
residual block is the oracle's Evaluate (O.eval_proj kinds 0 / 1 / 2, O.eval_imu_leg / O.eval_imu, O.eval_prior), enumerated as
Estimator::optimization adds them (estimator.cpp:1107-1216); the loss is O.huber. The reprojection sum is a literal transcription of
Estimator::outliersRejection / reprojectionError (estimator.cpp:1729-1798)."""
import numpy as np

from oracle import oracle_py as O

IMU_N = 31


def quat_R(q):
    """rotation matrix of a pose block's quaternion (x y z w), normalised first (Quaterniond(...).normalized().toRotationMatrix())"""
    x, y, z, w = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def reprojection_error(Ri, Pi, rici, tici, Rj, Pj, ricj, ticj, depth, uvi, uvj):
    """Estimator::reprojectionError (estimator.cpp:1729-1739)"""
    pts_w = Ri @ (rici @ (depth * uvi) + tici) + Pi
    pts_cj = ricj.T @ (Rj.T @ (pts_w - Pj) - ticj)
    residual = (pts_cj / pts_cj[2])[:2] - uvj[:2]
    rx, ry = residual
    return np.sqrt(rx * rx + ry * ry)


def landmark_reprojection(w, l):
    """(err, cnt) of outliersRejection for landmark l (its inner loop, estimator.cpp:1752-1790, STEREO on)"""
    s, o0, o1 = int(w.lm_start_frame[l]), int(w.lm_obs_offset[l]), int(w.lm_obs_offset[l + 1])
    R = [quat_R(w.pose[k][3:7]) for k in range(w.F)]
    P = [w.pose[k][0:3] for k in range(w.F)]
    ric = [quat_R(w.ex_pose[c][3:7]) for c in range(2)]
    tic = [w.ex_pose[c][0:3] for c in range(2)]
    err, cnt = 0.0, 0
    imu_i, imu_j = s, s - 1
    pts_i = w.obs[o0][0:3]
    depth = 1.0 / w.inv_depth[l]
    for o in range(o0, o1):
        imu_j += 1
        if imu_i != imu_j:
            err += reprojection_error(R[imu_i], P[imu_i], ric[0], tic[0], R[imu_j], P[imu_j], ric[0], tic[0], depth, pts_i, w.obs[o][0:3])
            cnt += 1
        if w.obs_is_stereo[o]:
            err += reprojection_error(R[imu_i], P[imu_i], ric[0], tic[0], R[imu_j], P[imu_j], ric[1], tic[1], depth, pts_i, w.obs[o][3:6])
            cnt += 1
    return err, cnt


def window_residuals(cfg, w, outlier_threshold_px=3.0):
    """Every output of vilo_batch_residuals for one window at its state arrays, as a dict: the vilo_window_residual fields, lm_cost,
    lm_reproj_px, lm_flags, obs_residuals [n_obs, 4] and imu_residuals [10, 31]."""
    delta = cfg.huber_delta
    st = {0: w.pose, 1: w.speed_bias, 2: w.leg_bias, 3: w.ex_pose, 4: w.td.reshape(1, 1)}
    out = dict(prior_cost=0.0, imu_cost=np.zeros(10), imu_residuals=np.zeros((10, IMU_N)))
    pr = w.prior
    if pr is not None and pr.struct.valid and pr.struct.n > 0:
        keys = [(pr.struct.block_id[k] // 16, pr.struct.block_id[k] % 16) for k in range(pr.struct.n_blocks)]
        r = O.eval_prior(pr.struct, [st[kind][idx] for kind, idx in keys], want_jac=False)[0]
        out["prior_cost"] = 0.5 * float(r @ r)
    for k in range(w.F - 1):
        if w.use_leg:
            if not (w.preint[k][0] <= 10.0):   # sum_dt > 10 s: no factor (estimator.cpp:1118)
                continue
            r = O.eval_imu_leg(cfg, w.preint[k], [w.pose[k], w.speed_bias[k], w.leg_bias[k], w.pose[k + 1], w.speed_bias[k + 1],
                                                  w.leg_bias[k + 1]], want_jac=False)[0]
        else:
            if not (w.preint_imu[k][0] <= 10.0):   # (estimator.cpp:1164)
                continue
            r = O.eval_imu(cfg, w.preint_imu[k], [w.pose[k], w.speed_bias[k], w.pose[k + 1], w.speed_bias[k + 1]], want_jac=False)[0]
        out["imu_residuals"][k, :len(r)] = r
        out["imu_cost"][k] = 0.5 * float(r @ r)
    L = w.L
    lm_cost, lm_plain, lm_px = np.zeros(L), np.zeros(L), np.zeros(L)
    lm_flags = np.zeros(L, np.uint8)
    obs_res = np.full((int(w.lm_obs_offset[L]) if L else 0, 4), np.nan)
    counts = dict(nb=0, nh=0)
    td = w.td
    for l in range(L):
        s, o0, o1 = int(w.lm_start_frame[l]), int(w.lm_obs_offset[l]), int(w.lm_obs_offset[l + 1])
        f0 = w.obs[o0]
        lam = w.inv_depth[l:l + 1]
        huber_on = False

        def add(r, o, col):
            nonlocal huber_on
            s2 = float(r @ r)
            lm_cost[l] += 0.5 * O.huber(delta, s2)[0]
            lm_plain[l] += 0.5 * s2
            obs_res[o, col:col + 2] = r
            counts["nb"] += 1
            if s2 > delta * delta:
                counts["nh"] += 1
                huber_on = True
        for o in range(o0, o1):
            j = s + (o - o0)
            fj = w.obs[o]
            if j != s:
                obs = np.concatenate([f0[0:3], fj[0:3], f0[6:8], fj[6:8], [f0[10], fj[10]]])
                add(O.eval_proj(0, cfg, obs, [w.pose[s], w.pose[j], w.ex_pose[0], lam, td], want_jac=False)[0], o, 0)
            if w.obs_is_stereo[o]:
                obs = np.concatenate([f0[0:3], fj[3:6], f0[6:8], fj[8:10], [f0[10], fj[10]]])
                if j != s:
                    add(O.eval_proj(1, cfg, obs, [w.pose[s], w.pose[j], w.ex_pose[0], w.ex_pose[1], lam, td], want_jac=False)[0], o, 2)
                else:
                    add(O.eval_proj(2, cfg, obs, [w.ex_pose[0], w.ex_pose[1], lam, td], want_jac=False)[0], o, 2)
        err, cnt = landmark_reprojection(w, l)
        with np.errstate(invalid="ignore", divide="ignore"):
            lm_px[l] = (err / cnt) * cfg.focal_length
        lm_flags[l] = (1 if lm_px[l] > outlier_threshold_px else 0) | (2 if 1.0 / w.inv_depth[l] < 0 else 0) | (4 if huber_on else 0)
    out.update(visual_cost=float(lm_cost.sum()), visual_cost_plain=float(lm_plain.sum()), n_visual_blocks=counts["nb"],
               n_huber_active=counts["nh"], n_outliers=int((lm_flags & 1).sum()), n_negative_depth=int(((lm_flags >> 1) & 1).sum()),
               status=0, lm_cost=lm_cost, lm_reproj_px=lm_px, lm_flags=lm_flags, obs_residuals=obs_res)
    out["cost"] = out["prior_cost"] + float(out["imu_cost"].sum()) + out["visual_cost"]
    return out


def shift_observations(w, landmarks, px, focal_length):
    """Moves the left-camera point of every non-start observation of the given landmarks by px pixels in x (in place; the inputs are
    copied first, so twins of w keep theirs)."""
    w.obs = w.obs.copy()
    for l in landmarks:
        o0, o1 = int(w.lm_obs_offset[l]), int(w.lm_obs_offset[l + 1])
        w.obs[o0 + 1:o1, 0] += px / focal_length
    return w
