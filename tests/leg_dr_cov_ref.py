"""Test helper (no test in it): the definition of vilo_batch_leg_dead_reckon_covariance (include/vilo_gpu.h, "covariance of a frame's
leg-odometry state carried through samples") in numpy, written from the reference's own lines: the noise diagonal, F and V of
IMULegIntegrationBase::midPointIntegration (imu_leg_integration_base.cpp:259-468), A1Kinematics' generated derivatives
(A1Kinematics.cpp:109-221) and the ILStateOrder / ILNoiseStateOrder indices (parameters.h:135-175). Nothing of
cerberus_amd/csrc/legdrcov_host.hpp: F (31 x 31) and V (31 x 46) are formed in full, block by block as the source writes them, and the
step is the three matrix products of :468, in `dtype` (float64, or numpy.longdouble for the FP64 floor).

The nominal state is tests/leg_dr_model.py's integrate(): result_delta_q, the flags and lo_v of every step are its rows; delta_q before a
step is the normalised result_delta_q of the step before (as integrate() carries it), delta_v before a step is integrate()'s delta_v of the
samples up to it, and the five-slot force variance, which integrate() keeps to itself, is restated from :200-222.

The world frame comes in by the substitutions the header states: delta_q.toRotationMatrix() -> R_f R(delta_q),
result_delta_q.toRotationMatrix() -> R_f R(result_delta_q), linearized_* -> the frame's biases.

`wrong` names one deliberate mistake (MISTAKES); tests/test_leg_dr_covariance.py asserts that each one moves the answer."""
import collections

import numpy as np

import leg_dr_model as L

N, N_IN, NOISE = 31, 19, 46
O_P, O_R, O_V, O_EPS, O_BA, O_BG, O_RHO = 0, 3, 6, 9, 21, 24, 27                       # ILStateOrder
N_AI, N_GI, N_AI1, N_GI1, N_BA, N_BG, N_PHII, N_PHII1, N_DPHII, N_DPHII1, N_V1, N_NRHO1 = 0, 3, 6, 9, 12, 15, 18, 21, 24, 27, 30, 42   # ILNoiseStateOrder
MISTAKES = ("no_vqv", "f_transposed", "pre_rotation", "acc_n_for_z", "q_flag_independent", "no_override", "phi_dphi_swapped",
            "no_rho_column", "unc_squared", "no_dp_eps")

# FP64 floor of the definition in the metric cov_error below (worst entry of |d Sigma_ij| / sqrt(Sigma_ii Sigma_jj) over cov_out and both
# trajectories): the restatement in float64 against numpy.longdouble, and every input moved one unit in the last place, over the cases of
# tests/test_leg_dr_covariance.py, as test_fp64_floor_measured prints it, rounded up. The all-feet-in-the-air case is measured on its
# own (its diagonal carries 1e11 dt^2 beside 1e-8-sized entries): it measures lower, not orders of magnitude apart, so one constant holds.
# Measured (x86-64): precision 1.9e-15, one-ulp inputs 1.0e-15; all feet in the air 7.5e-16 and 9.9e-16.
FLOOR = 2e-15
TOL = 10 * FLOOR

LegDrCov = collections.namedtuple("LegDrCov", "state legs cov pose_cov_trajectory leg_cov_trajectory n_steps status branches")


def _rot(q, dt):
    """Eigen's toRotationMatrix of (w, x, y, z), no normalisation"""
    w, x, y, z = q
    two = dt(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = dt(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, one - (txx + tyy)]], dtype=dt)


def _dfk_drho(q, dt):
    """autoFunc_d_fk_drho (A1Kinematics.cpp:109-120)"""
    t5 = q[1] + q[2]
    t6 = np.cos(t5)
    return np.array([-np.sin(t5), t6 * np.sin(q[0]), -t6 * np.cos(q[0])], dtype=dt)


def _dJ_dq(q, lc, rf, dt):
    """autoFunc_dJ_dt (:122-193): the 27 values, Eigen's column-major 9 x 3"""
    t5, t6, t7 = np.cos(q[0]), np.cos(q[1]), np.cos(q[2])
    t8, t9, t10 = np.sin(q[0]), np.sin(q[1]), np.sin(q[2])
    t11 = q[1] + q[2]
    t12 = rf[3] * t6
    t16 = lc * np.cos(t11)
    t17 = lc * np.sin(t11)
    t18 = t5 * t16
    t25 = t12 + t16
    t26 = rf[3] * t9 + t17
    t11 = -(t8 * t16)
    t16 = -(t5 * t17)
    t24 = -(t8 * t17)
    t29 = -(t5 * t26)
    t30 = -(t8 * t26)
    z = dt(0)
    tmp = lc * t5
    d = [z, ((-rf[2] * t5 - t8 * t12) - lc * t6 * t7 * t8) + lc * t8 * t9 * t10, ((-rf[2] * t8 + t5 * t12) + tmp * t6 * t7) - tmp * t9 * t10,
         z, t29, t30, z, t16, t24, z, t29, t30, t26, -t8 * t25, t5 * t25, t17, t11, t18, z, t16, t24, t17, t11, t18, t17, t11, t18]
    return np.array(d, dtype=dt).reshape(3, 9).T.copy()   # [9, 3]


def _dJ_drho(q, dt):
    """autoFunc_dJ_drho (:195-221): 9 x 1"""
    t5, t6 = np.cos(q[0]), np.sin(q[0])
    t7 = q[1] + q[2]
    t8 = np.cos(t7)
    t7 = np.sin(t7)
    t10 = t6 * t7
    t7 = t7 * t5
    return np.array([dt(0), t5 * t8, t6 * t8, -t8, -t10, t7, -t8, -t10, t7], dtype=dt).reshape(9, 1)


def _kron(dphi, dt):
    """kron_dphi (:267-271)"""
    k = np.zeros((3, 9), dt)
    for c in range(3):
        k[0, 3 * c] = k[1, 3 * c + 1] = k[2, 3 * c + 2] = dphi[c]
    return k


def embed(cov_in, dt, wrong=None):
    """Sigma_0 = E cov_in E^T from the upper triangle of cov_in [19, 19] (None: zeros)"""
    if cov_in is None:
        return np.zeros((N, N), dt)
    u = np.triu(np.asarray(cov_in, np.float64))
    full = (u + np.triu(u, 1).T).astype(dt)
    E = np.zeros((N, N_IN), dt)
    for i in range(9):
        E[i, i] = 1
    for i in range(10):
        E[O_BA + i, 9 + i] = 1
    if wrong != "no_dp_eps":
        for j in range(4):
            for a in range(3):
                E[O_EPS + 3 * j + a, a] = 1
    S = E @ full @ E.T
    return S


def propagate(cfg, lin, samples, R_f, Sigma0, dtype=np.float64, wrong=None):
    """Sigma after every step (list of [31, 31]) and the branches, for the constructor at lin = (ba, bg, rho) with samples[0] and push_back of
    samples[1:]; R_f: the world rotation of the frame ([3, 3], identity: the preintegration frame of the reference's record)"""
    dt_ = dtype
    c = lambda a: np.asarray(a, dtype=np.float64).astype(dt_)   # noqa: E731
    s = c(samples).reshape(-1, 35)
    lin = c(lin)
    ba, bg, rho = lin[0:3], lin[3:6], lin[6:10]
    rho_fix = c(np.ctypeslib.as_array(cfg.rho_fix).reshape(4, 4))
    p_br, R_br = c(np.ctypeslib.as_array(cfg.p_br)), c(np.ctypeslib.as_array(cfg.R_br).reshape(3, 3))
    kind = int(cfg.contact_sensor_type)
    k = lambda name: dt_(getattr(cfg, name))   # noqa: E731
    half, one, I3 = dt_(0.5), dt_(1), np.eye(3, dtype=dt_)
    R_f = c(R_f)
    nom = L.integrate(cfg, lin, samples, dtype)
    Sigma = Sigma0.astype(dt_)
    out = []
    f_win, f_idx, f_var = np.zeros((4, 5), dt_), np.zeros(4, int), np.zeros(4, dt_)
    br = dict(all_air=0, clamped=0, flags=[])
    for i in range(1, len(s)):
        st = nom["steps"][i - 1]
        dt = s[i, 0]
        acc_0, gyr_0, acc_1, gyr_1 = s[i - 1, 1:4], s[i - 1, 4:7], s[i, 1:4], s[i, 4:7]
        phi_0, dphi_0, c_0, phi_1, dphi_1, c_1 = s[i - 1, 7:19], s[i - 1, 19:31], s[i - 1, 31:35], s[i, 7:19], s[i, 19:31], s[i, 31:35]
        if i == 1:
            dq = (one, dt_(0), dt_(0), dt_(0))
        else:
            p = nom["steps"][i - 2]["rq"]
            n = np.sqrt(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] + p[3] * p[3])
            dq = (p[0] / n, p[1] / n, p[2] / n, p[3] / n)
        rq = st["rq"]
        delta_v = L.integrate(cfg, lin, samples[:i], dtype)["dv"] if i > 1 else np.zeros(3, dt_)
        Rq = R_f @ _rot(dq, dt_)
        Rrq = Rq if wrong == "pre_rotation" else R_f @ _rot(rq, dt_)
        flag = st["flag"]
        # :200-222, the variance of the five-slot window alone
        if kind == 2:
            for j in range(4):
                force_mag = half * (c_0[j] + c_1[j])
                f_idx[j] = (f_idx[j] + 1) % 5
                f_win[j, f_idx[j]] = force_mag
                mean = dt_(0)
                for y in f_win[j]:
                    mean = mean + y
                mean = mean / dt_(5)
                ss = dt_(0)
                for y in f_win[j]:
                    ss = ss + (y - mean) * (y - mean)
                f_var[j] = ss / dt_(4)
        R_w_0_x, R_w_1_x = L._skew(gyr_0 - bg, dt_), L._skew(gyr_1 - bg, dt_)
        fi, fip1, Ji, Jip1, vi, vip1, gi, gip1, hi, hip1 = [], [], [], [], [], [], [], [], [], []
        for j in range(4):
            q0, q1, d0, d1 = phi_0[3 * j:3 * j + 3], phi_1[3 * j:3 * j + 3], dphi_0[3 * j:3 * j + 3], dphi_1[3 * j:3 * j + 3]
            fi.append(L._fk(q0, rho[j], rho_fix[j], dt_)); fip1.append(L._fk(q1, rho[j], rho_fix[j], dt_))
            Ji.append(L._jac(q0, rho[j], rho_fix[j], dt_)); Jip1.append(L._jac(q1, rho[j], rho_fix[j], dt_))
            vi.append(-R_br @ Ji[j] @ d0 - R_w_0_x @ (p_br + R_br @ fi[j]))                      # :242
            vip1.append(-R_br @ Jip1[j] @ d1 - R_w_1_x @ (p_br + R_br @ fip1[j]))                # :243
            dfdrhoi, dfdrhoip1 = _dfk_drho(q0, dt_).reshape(3, 1), _dfk_drho(q1, dt_).reshape(3, 1)
            gi.append(-Rq @ (R_br @ _kron(d0, dt_) @ _dJ_drho(q0, dt_) + R_w_0_x @ R_br @ dfdrhoi))       # :272
            gip1.append(-Rrq @ (R_br @ _kron(d1, dt_) @ _dJ_drho(q1, dt_) + R_w_1_x @ R_br @ dfdrhoip1))  # :280
            hi.append(Rq @ (R_br @ _kron(d0, dt_) @ _dJ_dq(q0, rho[j], rho_fix[j], dt_) + R_w_0_x @ R_br @ Ji[j]))       # :284
            hip1.append(Rrq @ (R_br @ _kron(d1, dt_) @ _dJ_dq(q1, rho[j], rho_fix[j], dt_) + R_w_1_x @ R_br @ Jip1[j]))  # :286
        # :288-322
        qflag = np.ones(4, dt_) if wrong == "q_flag_independent" else flag
        unc = np.zeros(12, dt_)
        for j in range(4):
            if kind in (0, 1):
                n_xy = k("v_n_max") * (one - qflag[j]) + qflag[j] * k("v_n_min_xy")
                n_z = k("v_n_max") * (one - qflag[j]) + qflag[j] * k("v_n_min_z")
                unc[3 * j:3 * j + 3] = (n_xy, n_xy, n_z)
            else:
                n1 = k("v_n_max") * (one - qflag[j]) + k("v_n_min")
                n2 = k("v_n_term2_var_rescale") * f_var[j]
                tmp = st["lo_v"][j] - delta_v
                unc[3 * j:3 * j + 3] = (n1 + n2) + k("v_n_term3_distance_rescale") * (tmp * tmp)
        rho_unc = np.array([k("rho_c_n") * qflag[j] + k("rho_nc_n") for j in range(4)], dtype=dt_)
        all_air = bool(qflag.sum() < 1e-6)   # :354
        if all_air and wrong != "no_override":
            rho_unc[:] = k("rho_nc_n")
            unc[:] = dt_(10e10)
        br["all_air"] += int(bool(flag.sum() < 1e-6)); br["clamped"] += st["clamped"]; br["flags"].append(np.asarray(flag, np.float64))
        if wrong == "unc_squared":
            unc = unc * unc
        acc_n2, gyr_n2 = k("acc_n") * k("acc_n"), k("gyr_n") * k("gyr_n")
        acc_nz2 = acc_n2 if wrong == "acc_n_for_z" else k("acc_n_z") * k("acc_n_z")
        phi2, dphi2 = k("phi_n") * k("phi_n"), k("dphi_n") * k("dphi_n")
        if wrong == "phi_dphi_swapped":
            phi2, dphi2 = dphi2, phi2
        Q = np.concatenate([[acc_n2, acc_n2, acc_nz2], [gyr_n2] * 3, [acc_n2, acc_n2, acc_nz2], [gyr_n2] * 3, [k("acc_w") * k("acc_w")] * 3,
                            [k("gyr_w") * k("gyr_w")] * 3, [phi2] * 6, [dphi2] * 6, unc, rho_unc]).astype(dt_)   # :360-374
        # :378-465
        w_x = half * (gyr_0 + gyr_1) - bg
        R_w_x, R_a_0_x, R_a_1_x = L._skew(w_x, dt_), L._skew(acc_0 - ba, dt_), L._skew(acc_1 - ba, dt_)
        kappa_7 = I3 - R_w_x * dt
        F = np.zeros((N, N), dt_)
        F[O_P:O_P + 3, O_P:O_P + 3] = I3
        kappa_1 = -half * Rq @ R_a_0_x * dt + -half * Rrq @ R_a_1_x @ kappa_7 * dt
        F[O_P:O_P + 3, O_R:O_R + 3] = half * dt * kappa_1
        F[O_P:O_P + 3, O_V:O_V + 3] = I3 * dt
        F[O_P:O_P + 3, O_BA:O_BA + 3] = -dt_(0.25) * (Rq + Rrq) * dt * dt
        F[O_P:O_P + 3, O_BG:O_BG + 3] = dt_(0.25) * Rrq @ R_a_1_x * dt * dt * dt
        F[O_R:O_R + 3, O_R:O_R + 3] = kappa_7
        F[O_R:O_R + 3, O_BG:O_BG + 3] = -one * I3 * dt
        F[O_V:O_V + 3, O_R:O_R + 3] = kappa_1
        F[O_V:O_V + 3, O_V:O_V + 3] = I3
        F[O_V:O_V + 3, O_BA:O_BA + 3] = -half * (Rq + Rrq) * dt
        F[O_V:O_V + 3, O_BG:O_BG + 3] = half * Rrq @ R_a_1_x * dt * dt
        V = np.zeros((N, NOISE), dt_)
        for j in range(4):
            e = O_EPS + 3 * j
            pi, pip1 = L._skew(p_br + R_br @ fi[j], dt_), L._skew(p_br + R_br @ fip1[j], dt_)
            F[e:e + 3, O_R:O_R + 3] = -half * dt * Rq @ L._skew(vi[j], dt_) - half * dt * Rrq @ L._skew(vip1[j], dt_) @ kappa_7
            F[e:e + 3, e:e + 3] = I3
            F[e:e + 3, O_BG:O_BG + 3] = half * dt * dt * Rrq @ L._skew(vip1[j], dt_) - half * dt * (Rq @ pi + Rrq @ pip1)
            if wrong != "no_rho_column":
                F[e:e + 3, O_RHO + j:O_RHO + j + 1] = half * dt * (gi[j] + gip1[j])
            V[e:e + 3, N_GI:N_GI + 3] = -dt_(0.25) * dt * dt * Rrq @ L._skew(vip1[j], dt_) + half * dt * Rq @ pi
            V[e:e + 3, N_GI1:N_GI1 + 3] = -dt_(0.25) * dt * dt * Rrq @ L._skew(vip1[j], dt_) + half * dt * Rrq @ pip1
            V[e:e + 3, N_PHII:N_PHII + 3] = -half * dt * hi[j]
            V[e:e + 3, N_PHII1:N_PHII1 + 3] = -half * dt * hip1[j]
            V[e:e + 3, N_DPHII:N_DPHII + 3] = -half * dt * Rq @ R_br @ Ji[j]
            V[e:e + 3, N_DPHII1:N_DPHII1 + 3] = -half * dt * Rrq @ R_br @ Jip1[j]
            # :456 is -I dt in frame f's body frame, whose axes the uncertainties belong to (n_xy is not n_z): in the world frame -R_f dt
            V[e:e + 3, N_V1 + 3 * j:N_V1 + 3 * j + 3] = -R_f * dt
            V[O_RHO + j, N_NRHO1 + j] = -dt
        for b in (O_BA, O_BG, O_RHO):
            F[b:b + 3, b:b + 3] = I3
        F[O_RHO + 3, O_RHO + 3] = one
        V[O_P:O_P + 3, N_AI:N_AI + 3] = dt_(0.25) * Rq * dt * dt
        V[O_P:O_P + 3, N_GI:N_GI + 3] = dt_(0.25) * -Rrq @ R_a_1_x * dt * dt * half * dt
        V[O_P:O_P + 3, N_AI1:N_AI1 + 3] = dt_(0.25) * Rrq * dt * dt
        V[O_P:O_P + 3, N_GI1:N_GI1 + 3] = V[O_P:O_P + 3, N_GI:N_GI + 3]
        V[O_R:O_R + 3, N_GI:N_GI + 3] = half * I3 * dt
        V[O_R:O_R + 3, N_GI1:N_GI1 + 3] = half * I3 * dt
        V[O_V:O_V + 3, N_AI:N_AI + 3] = half * Rq * dt
        V[O_V:O_V + 3, N_GI:N_GI + 3] = half * -Rrq @ R_a_1_x * dt * half * dt
        V[O_V:O_V + 3, N_AI1:N_AI1 + 3] = half * Rrq * dt
        V[O_V:O_V + 3, N_GI1:N_GI1 + 3] = V[O_V:O_V + 3, N_GI:N_GI + 3]
        V[O_BA:O_BA + 3, N_BA:N_BA + 3] = -I3 * dt
        V[O_BG:O_BG + 3, N_BG:N_BG + 3] = -I3 * dt
        if wrong == "f_transposed":
            F = F.T.copy()
        Sigma = F @ Sigma @ F.T                                   # :468
        if wrong != "no_vqv":
            Sigma = Sigma + (V * Q[None, :]) @ V.T
        out.append(Sigma)
    br["flags"] = np.array(br["flags"], dtype=np.float64).reshape(-1, 4)
    return out, br


def sym(S):
    """a result as the call stores it: both halves from the upper triangle"""
    u = np.triu(S)
    return u + np.triu(u, 1).T


def window_leg_dr_cov(cfg, w, samples, from_frame=-1, cov_in=None, dtype=np.float64, wrong=None):
    """LegDrCov of one window at its state arrays through samples [n, 35]; cov_in: None or [19, 19]"""
    samples = np.asarray(samples, float).reshape(-1, 35)
    nom = L.window_leg_dead_reckon(cfg, w, samples, from_frame, dtype)
    n_steps = nom.n_steps
    zero = LegDrCov(np.zeros(L.STATE), np.zeros((4, 3)), np.zeros((N, N)), np.zeros((n_steps, 6, 6)), np.zeros((n_steps, 4, 3, 3)), n_steps, nom.status, {})
    if nom.status != L.OK:
        return zero
    if cov_in is not None and not np.isfinite(np.triu(np.asarray(cov_in, float))).all():
        return zero._replace(status=L.NUMERIC)
    f = w.F - 1 if from_frame == -1 else from_frame
    import deadreckon_ref as D
    R_f = D.quat_R(D.quat_normalized(np.asarray(w.pose[f, 3:7], np.float64).astype(dtype), dtype), dtype)
    lin = np.concatenate([w.speed_bias[f, 3:9], w.leg_bias[f, 0:4]])
    S0 = embed(cov_in, dtype, wrong)
    steps, br = propagate(cfg, lin, samples if n_steps else samples[:0], R_f, S0, dtype, wrong) if n_steps else ([], {})
    cov = sym((steps[-1] if steps else S0).astype(np.float64))
    if not np.isfinite(cov).all():
        return zero._replace(status=L.NUMERIC)
    pose = np.array([sym(S.astype(np.float64))[0:6, 0:6] for S in steps]).reshape(-1, 6, 6)
    legs = np.array([[sym(S.astype(np.float64))[O_EPS + 3 * j:O_EPS + 3 * j + 3, O_EPS + 3 * j:O_EPS + 3 * j + 3] for j in range(4)] for S in steps]).reshape(-1, 4, 3, 3)
    return LegDrCov(nom.state, nom.legs, cov, pose, legs, n_steps, L.OK, br)


def T_of(R_f, dt=np.float64):
    """T = blkdiag(R_f, I3, R_f, R_f x 4, I3, I3, I4)"""
    T = np.eye(N, dtype=dt)
    for o in (O_P, O_V, O_EPS, O_EPS + 3, O_EPS + 6, O_EPS + 9):
        T[o:o + 3, o:o + 3] = R_f
    return T


def from_record(rec, R_f, Sigma0, dt=np.float64):
    """T (Phi Sigma_0' Phi^T + Sigma_rec) T^T of a preintegration record (oracle_py.Preint layout: jacobian at 33, covariance at 994)"""
    rec = np.asarray(rec, np.float64).astype(dt)
    Phi, Srec = rec[33:33 + 961].reshape(N, N), rec[994:994 + 961].reshape(N, N)
    T = T_of(np.asarray(R_f, np.float64).astype(dt), dt)
    S0p = T.T @ Sigma0.astype(dt) @ T
    return T @ (Phi @ S0p @ Phi.T + Srec) @ T.T


def _rel(got, ref):
    got, ref = np.asarray(got, np.longdouble), np.asarray(ref, np.longdouble)
    d = np.sqrt(np.abs(np.diagonal(ref, axis1=-2, axis2=-1)))
    den = d[..., :, None] * d[..., None, :]
    diff = np.abs(got - ref)
    if not diff.size:
        return 0.0
    if (diff[den == 0] != 0).any():
        return float("inf")
    return float((diff[den > 0] / den[den > 0]).max()) if (den > 0).any() else 0.0


def cov_error(got, ref):
    """the metric: worst |d Sigma_ij| / sqrt(Sigma_ii Sigma_jj) over cov and both trajectories; got, ref: (cov, pose_traj, leg_traj). An
    entry whose row or column has a zero variance in the reference must agree exactly."""
    return max(_rel(got[0], ref[0]), _rel(got[1], ref[1]), _rel(got[2], ref[2]))
