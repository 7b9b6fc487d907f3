"""Test helper: the definition of vilo_batch_dead_reckon_covariance (include/vilo_gpu.h, "covariance of a frame's state carried through
IMU samples") in numpy, FP64, written from the header's text and IntegrationBase::midPointIntegration (integration_base.h:87-137): the
nominal step is tests/deadreckon_ref.py's, F (15 x 15), V (15 x 18) and Q (18 x 18) are built per step, block by block as the reference
writes them, and the triple product is plain `@`. Nothing of the kernel under test."""
import collections

import numpy as np

import deadreckon_ref as D

OK, NO_FRAME, NUMERIC = D.OK, D.NO_FRAME, D.NUMERIC
N, POSE = 15, 6
WRONG = ("no_noise", "F_transposed", "R_pre", "swap_bias_columns", "acc_w_for_gyr_w")

# FP64 floor of the definition, as tests/test_dr_covariance.py::test_fp64_floor_measured prints it over every case of the GPU parity test
# at both configurations, at the longest range any test uses (30 samples, 29 steps): the larger of (a) every start-state value, sample
# value and read cov_in entry moved by one unit in the last place and (b) the same recurrence in numpy.longdouble, rounded at the end.
# Metric: |dS_ij| / sqrt(S_ii S_jj), worst entry. Measured (x86-64): (a) 5.0e-14, (b) 6.2e-14, both on the solved six-frame window
# without a prior from its last frame, whose frame block is the most strongly correlated cov_in of the cases (the same window from frame
# 4: 5e-15; every other case, cov_in = 0 or the solved 11-frame windows': (a) at most 1.0e-15, (b) at most 2.3e-15); rounded up. The GPU
# tolerance is ten times the floor.
FLOOR = 1e-13
TOL = 10 * FLOOR

# Largest difference (the same metric) between cov_out of interval k - 1's own samples from frame k - 1 with cov_in = 0 and
# T S_rec T^T, S_rec the covariance of the oracle's IMU preintegration record of that interval and T = blkdiag(R_0, I, R_0, I, I), as
# tests/test_dr_covariance.py::test_tie_to_the_pinned_preintegration measures it on a CPU. It is not rounding: the record chains a
# NORMALISED quaternion, the dead reckoning an un-normalised matrix, and the two differ at third order in |un_gyr dt| per step (DESIGN
# §4.21 measured 1.4e-9 on the state; on the covariance, which the rotation enters through the noise maps alone, 8.1e-12 with a general
# R_0 and with R_0 = I alike). The test is gated at twice this value.
RECORD_DIFF = 8.1e-12

Noise = collections.namedtuple("Noise", "acc_n gyr_n acc_w gyr_w")
DrCov = collections.namedtuple("DrCov", "state cov pose_cov_trajectory n_steps status")


def noise_of(cfg):
    """the fields of a vilo_config (or of anything with those attributes) that Q reads; acc_n_z is not among them"""
    return Noise(float(cfg.acc_n), float(cfg.gyr_n), float(cfg.acc_w), float(cfg.gyr_w))


def skew(v, dtype=np.float64):
    z = dtype(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=dtype)


def mirrored(c, dtype=np.float64):
    """the upper triangle with the diagonal, and its mirror below"""
    c = np.asarray(c, dtype=np.float64).astype(dtype).reshape(N, N)
    return np.triu(c) + np.triu(c, 1).T


def step_matrices(R0, R1, un_gyr, a0, a1, dt, noise, dtype=np.float64, wrong=None):
    """(F, V, Q) of one step, integration_base.h:87-132 with delta_q.toRotationMatrix() -> R0 and result_delta_q.toRotationMatrix() -> R1"""
    I = np.eye(3, dtype=dtype)
    q, h, one = dtype(0.25), dtype(0.5), dtype(1)
    if wrong == "R_pre":
        R1 = R0
    R_w_x, R_a_0_x, R_a_1_x = skew(un_gyr, dtype), skew(a0, dtype), skew(a1, dtype)
    F = np.zeros((N, N), dtype=dtype)
    F[0:3, 0:3] = I
    F[0:3, 3:6] = -q * R0 @ R_a_0_x * dt * dt + -q * R1 @ R_a_1_x @ (I - R_w_x * dt) * dt * dt
    F[0:3, 6:9] = I * dt
    F[0:3, 9:12] = -q * (R0 + R1) * dt * dt
    F[0:3, 12:15] = -q * R1 @ R_a_1_x * dt * dt * -dt
    F[3:6, 3:6] = I - R_w_x * dt
    F[3:6, 12:15] = -one * I * dt
    F[6:9, 3:6] = -h * R0 @ R_a_0_x * dt + -h * R1 @ R_a_1_x @ (I - R_w_x * dt) * dt
    F[6:9, 6:9] = I
    F[6:9, 9:12] = -h * (R0 + R1) * dt
    F[6:9, 12:15] = -h * R1 @ R_a_1_x * dt * -dt
    F[9:12, 9:12] = I
    F[12:15, 12:15] = I
    V = np.zeros((N, 18), dtype=dtype)
    V[0:3, 0:3] = q * R0 * dt * dt
    V[0:3, 3:6] = q * -R1 @ R_a_1_x * dt * dt * h * dt
    V[0:3, 6:9] = q * R1 * dt * dt
    V[0:3, 9:12] = V[0:3, 3:6]
    V[3:6, 3:6] = h * I * dt
    V[3:6, 9:12] = h * I * dt
    V[6:9, 0:3] = h * R0 * dt
    V[6:9, 3:6] = h * -R1 @ R_a_1_x * dt * h * dt
    V[6:9, 6:9] = h * R1 * dt
    V[6:9, 9:12] = V[6:9, 3:6]
    V[9:12, 12:15] = I * dt
    V[12:15, 15:18] = I * dt
    an, gn, aw, gw = (dtype(x) for x in noise)
    if wrong == "acc_w_for_gyr_w":
        gw = aw
    Q = np.diag(np.repeat(np.array([an * an, gn * gn, an * an, gn * gn, aw * aw, gw * gw], dtype=dtype), 3))
    if wrong == "F_transposed":
        F = F.T.copy()
    if wrong == "swap_bias_columns":
        F[:, 9:12], F[:, 12:15] = F[:, 12:15].copy(), F[:, 9:12].copy()
    if wrong == "no_noise":
        Q = np.zeros_like(Q)
    return F, V, Q


def recurrence(P, q, V, ba, bg, g_norm, rows, cov, noise, dtype=np.float64, wrong=None):
    """(state [10], cov [15, 15], pose trajectory [max(0, n - 1), 6, 6]) in `dtype`: the nominal step of deadreckon_ref.recurrence, and
    S <- F S F^T + V Q V^T beside it"""
    c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)   # noqa: E731
    P, V, ba, bg, rows = c(P), c(V), c(ba), c(bg), c(rows).reshape(-1, 7)
    half, two = dtype(0.5), dtype(2)
    g = np.array([0, 0, g_norm], dtype=np.float64).astype(dtype)
    R = D.quat_R(D.quat_normalized(c(q), dtype), dtype)
    S = cov.astype(dtype)
    traj = []
    for i in range(1, len(rows)):
        dt, acc_0, gyr_0, acc_1, gyr_1 = rows[i, 0], rows[i - 1, 1:4], rows[i - 1, 4:7], rows[i, 1:4], rows[i, 4:7]
        R0 = R
        un_acc_0 = D._mv(R, acc_0 - ba) - g
        un_gyr = (gyr_0 + gyr_1) * half - bg
        th = un_gyr * dt
        R = D._mm(R, D.quat_R([th[0] / two, th[1] / two, th[2] / two, dtype(1)], dtype))
        un_acc_1 = D._mv(R, acc_1 - ba) - g
        un_acc = (un_acc_0 + un_acc_1) * half
        P = P + (V * dt + un_acc * (half * dt * dt))
        V = V + un_acc * dt
        F, Vm, Q = step_matrices(R0, R, un_gyr, acc_0 - ba, acc_1 - ba, dt, noise, dtype, wrong)
        S = F @ S @ F.T + Vm @ Q @ Vm.T
        traj.append(S[:POSE, :POSE])
    return D.state_row(P, R, V, dtype), S, traj


def sym(S):
    """stored from the upper triangle: bitwise symmetric"""
    S = np.asarray(S)
    return np.triu(S) + np.triu(S, 1).swapaxes(-1, -2)


def window_dr_cov(w, samples, g_norm, noise, from_frame=-1, cov_in=None, dtype=np.float64, wrong=None):
    """DrCov of one window at its state arrays through samples [n, 35] from cov_in [15, 15] (None: zero)"""
    rows = np.asarray(samples, float).reshape(-1, 35)[:, D.ROW]
    n_steps = max(0, len(rows) - 1)
    zero = DrCov(np.zeros(10), np.zeros((N, N)), np.zeros((n_steps, POSE, POSE)), n_steps, NO_FRAME)
    f = w.F - 1 if from_frame == -1 else from_frame
    if f >= w.F:
        return zero
    start = [w.pose[f, 0:3], w.pose[f, 3:7], w.speed_bias[f, 0:3], w.speed_bias[f, 3:6], w.speed_bias[f, 6:9]]
    read = np.concatenate([rows[:1, 1:].ravel(), rows[1:].ravel()]) if n_steps else np.zeros(0)   # (the first row's dt is not read)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        c0 = np.zeros((N, N)) if cov_in is None else mirrored(np.where(np.triu(np.ones((N, N), bool)), np.asarray(cov_in, float).reshape(N, N), 0.0))
        state, S, traj = recurrence(*start, g_norm, rows, c0, noise, dtype, wrong)
    ok = all(np.isfinite(a).all() for a in start) and np.isfinite(read).all() and np.isfinite(c0).all()
    if not (ok and np.isfinite(state.astype(float)).all() and np.isfinite(S.astype(float)).all()):
        return zero._replace(status=NUMERIC)
    t = sym(np.array(traj, dtype=dtype).astype(np.float64)) if traj else np.zeros((0, POSE, POSE))
    return DrCov(state.astype(np.float64), sym(S.astype(np.float64)), t, n_steps, OK)


def cov_error(got, ref):
    """|dS_ij| / sqrt(S_ii S_jj), worst entry, of covariances [n, n] (an entry whose scale is zero must be equal)"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    assert got.shape == ref.shape
    d = np.sqrt(np.abs(np.diag(ref)))
    scale = d[:, None] * d[None, :]
    diff = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(diff == 0.0, 0.0, diff / scale)
    return float(np.nan_to_num(e, nan=np.inf).max())


def rows_error(got, ref):
    assert np.shape(got) == np.shape(ref)
    return max([cov_error(a, b) for a, b in zip(got, ref)], default=0.0)
