"""Test helper: the landmark covariance of a window (include/vilo_gpu.h, "landmark covariance") in numpy, from the full covariance of
ref_gradient.dense_jacobian's problem with the inverse depths kept (their columns, keys (9, l), come last) — the landmark rows of
Sigma_full = N (N^T H N)^-1 N^T, or H^-1 under the NONE gauge. Returns what vilo_batch_landmark_covariance returns for one window, in the
caller's landmark order: inv_depth_var [L], points [L][3] (pubPointCloud's point), point_cov [L][3][3]."""
import numpy as np

import cov_ref
from ref_gradient import dense_jacobian  # noqa: F401  (cov_ref.hessian's Jacobian: the definition's only input)

# GPU tolerances, at least ten times the FP64 floor tests/test_landmark_covariance.py measures (a one-ulp perturbation of J, and one small window
# against 40-digit arithmetic): inverse-depth variance relative, point covariance correlation-scaled (|dS_ij| / sqrt(S_ii S_jj)).
# With a prior: variance 3.1e-7 (FRAME0) / 9.5e-7 (NONE), point covariance 3.5e-7 / 1.0e-6 under the one-ulp perturbation; 4.1e-7 /
# 5.1e-7 against 40 digits. Without a prior (only the FRAME0 gauge holds the window; cond ~1e13): variance 7.4e-6, point covariance
# 1.9e-4. (The elimination form from E, w and Sigma_PP agrees with the full inverse to 2e-11.)
TOL_VAR, TOL_PCOV = 1e-5, 2e-5
TOL_VAR_NO_PRIOR, TOL_PCOV_NO_PRIOR = 1e-4, 2e-3
TOL_POINT = 1e-12   # the world point, relative to its norm: the same formula in FP64 on both sides


def tolerances(has_prior):
    """(inverse-depth variance, point covariance)"""
    return (TOL_VAR, TOL_PCOV) if has_prior else (TOL_VAR_NO_PRIOR, TOL_PCOV_NO_PRIOR)


def quat_mul(a, b):
    """[x y z w] quaternions, Eigen's a * b"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def pose_plus(x, d):
    """PoseLocalParameterization::Plus: p + dp, normalise(q * [dtheta / 2, 1])"""
    q = quat_mul(x[3:7], np.array([d[3] / 2.0, d[4] / 2.0, d[5] / 2.0, 1.0]))
    return np.concatenate([x[:3] + d[:3], q / np.linalg.norm(q)])


def skew(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def first_observation(w, l):
    return np.asarray(w.obs[int(w.lm_obs_offset[l])][0:3], float)


def world_point(pose_s, ex0, f, rho):
    """pubPointCloud: R_s (R_c f / rho + t_c) + P_s"""
    Rs, Rc = cov_ref.quat_R(pose_s[3:7]), cov_ref.quat_R(ex0[3:7])
    return Rs @ (Rc @ (f / rho) + ex0[:3]) + pose_s[:3]


def world_points(w):
    return np.array([world_point(w.pose[int(w.lm_start_frame[l])], w.ex_pose[0], first_observation(w, l), w.inv_depth[l]) for l in range(w.L)]).reshape(-1, 3)


def point_jacobian(pose_s, ex0, f, rho):
    """3 x 13 derivative of the world point over [dp_s dtheta_s dt_c dtheta_c rho] (PoseLocalParameterization's local coordinates)"""
    Rs, Rc = cov_ref.quat_R(pose_s[3:7]), cov_ref.quat_R(ex0[3:7])
    a = f / rho
    b = Rc @ a + ex0[:3]
    J = np.zeros((3, 13))
    J[:, 0:3] = np.eye(3)
    J[:, 3:6] = -Rs @ skew(b)
    J[:, 6:9] = Rs
    J[:, 9:12] = -Rs @ Rc @ skew(a)
    J[:, 12] = -Rs @ Rc @ f / rho ** 2
    return J


def joint_index(cols, s):
    """columns of [dp_s dtheta_s dt_c dtheta_c] in dense_jacobian's layout (None where the block is constant)"""
    out = [cols[(0, s)].start + c for c in range(6)]
    out += [cols[(3, 0)].start + c for c in range(6)] if (3, 0) in cols else [None] * 6
    return out


def outputs(S, cols, w):
    """inv_depth_var [L], points [L][3], point_cov [L][3][3] from a full covariance S over dense_jacobian's columns"""
    L = w.L
    var, pcov = np.zeros(L), np.zeros((L, 3, 3))
    pts = world_points(w)
    for l in range(L):
        s, cl = int(w.lm_start_frame[l]), cols[(9, l)].start
        idx = joint_index(cols, s) + [cl]
        C = np.zeros((13, 13))
        for i, ii in enumerate(idx):
            for j, jj in enumerate(idx):
                if ii is not None and jj is not None:
                    C[i, j] = S[ii, jj]
        J = point_jacobian(w.pose[s], w.ex_pose[0], first_observation(w, l), w.inv_depth[l])
        var[l] = S[cl, cl]
        pcov[l] = J @ C @ J.T
    return var, pts, pcov


def full_covariance(cfg, w, gauge="frame0", J=None):
    """(Sigma_full, cols, H) with the inverse depths kept; J: a perturbed copy of the Jacobian to use instead"""
    H, cols, J0 = cov_ref.hessian(cfg, w)
    if J is not None:
        H = J.T @ J
    N = cov_ref.gauge_basis(w, cols, H.shape[0]) if gauge == "frame0" else None
    return cov_ref.covariance(H, N), cols, H


def landmark_covariance(cfg, w, gauge="frame0"):
    S, cols, _ = full_covariance(cfg, w, gauge)
    return outputs(S, cols, w)


def pose_system_coupling(H, cols, l):
    """(E, w [79]): H_ll and H_{P,l} in the pose system's layout (11 poses, ex0, ex1, td; zero where a block is constant or absent)"""
    ix = cov_ref.camera_index(cols)
    cl = cols[(9, l)].start
    wv = np.zeros(79)
    for p in range(79):
        if ("p", p) in ix:
            wv[p] = H[ix[("p", p)], cl]
    return H[cl, cl], wv


def schur_form(E, wv, Spp):
    """(Sigma_rr, Sigma_rP [79]) from E, w and Sigma_PP: the definition's elimination form"""
    u = Spp @ wv
    return 1.0 / E + wv @ u / E ** 2, -u / E


def errors(var_a, pcov_a, var_b, pcov_b):
    """worst relative difference of the variances and worst correlation-scaled difference of the point covariances (b: the reference)"""
    ev = float(np.max(np.abs(var_a - var_b) / np.abs(var_b))) if len(var_b) else 0.0
    ep = float(cov_ref.scaled_diff(pcov_a, pcov_b).max()) if len(var_b) else 0.0
    return {"var": ev, "pcov": ep}
