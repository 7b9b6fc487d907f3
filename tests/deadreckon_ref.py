"""Test helper: the definition of vilo_batch_dead_reckon (include/vilo_gpu.h, "mid-point dead reckoning of a frame's state through IMU
samples") in numpy, FP64, written from the header's text and Estimator::processIMULeg (estimator.cpp:639-646): the recurrence, the state
row, the statuses of one window. Every product and sum is a numpy elementwise operation in the order the header writes it (no BLAS call,
which may fuse), so the definition rounds where the formula does. Nothing of the kernel under test."""
import collections

import numpy as np

OK, NO_FRAME, NUMERIC = 0, 1, 2
ROW = slice(0, 7)   # dt acc gyr of a vilo_sample row of 35 doubles

# FP64 floor of the definition, as tests/test_dead_reckon.py::test_fp64_floor_measured prints it over every case of the GPU parity test,
# at the longest range any test uses (30 samples, 29 steps): the largest of (a) every start-state value and every sample value moved by
# one unit in the last place and (b) the same recurrence in numpy.longdouble, rounded at the end. Metric: |dP|inf / max(1, |P|inf), the
# same for V, and |dR|inf on the rotation matrix of the returned quaternion (so that its sign does not enter). Measured (x86-64):
# (a) P 1.1e-16, V 2.2e-16, R 1.1e-16; (b) P 2.2e-16, V 2.2e-16, R 1.1e-16: one unit in the last place of 1.0 (the synthetic robot's
# positions and velocities are below 1 in magnitude over these ranges, so the metric's max(1, .) is 1); rounded up to one digit. The
# GPU tolerance is ten times the floor.
FLOOR = 3e-16
TOL = 10 * FLOOR

# Largest difference (the same metric) between the dead-reckoned state of interval k - 1's own samples from frame k - 1 and the state
# composed from the oracle's preintegration record of that interval, P_i + V_i T - 1/2 g T^2 + R_i dp, V_i - g T + R_i dv, R_i R(dq), as
# tests/test_dead_reckon.py::test_tie_to_the_pinned_preintegration measures it on a CPU. It is not rounding: the record chains a
# NORMALISED quaternion in the body frame, the dead reckoning an un-normalised matrix in the world frame, and the two differ at third
# order in |un_gyr dt| per step (measured 1.4e-9 where sum |gyr dt|^3 reaches 4.6e-9). The test is gated at twice this
# value.
RECORD_DIFF = 1.4e-9

DeadReckoned = collections.namedtuple("DeadReckoned", "state trajectory n_steps status")


def quat_R(q, dtype=np.float64):
    """Eigen toRotationMatrix of [x y z w], no normalisation (vilo_math.hpp qR)"""
    x, y, z, w = (dtype(v) for v in q)
    two = dtype(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    one = dtype(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], dtype=dtype)


def quat_normalized(q, dtype=np.float64):
    x, y, z, w = (dtype(v) for v in q)
    n = np.sqrt(w * w + x * x + y * y + z * z)
    return np.array([x / n, y / n, z / n, w / n], dtype=dtype)


def quat_from_R(m, dtype=np.float64):
    """Eigen::Quaterniond(Matrix3d) as [x y z w]"""
    half, one = dtype(0.5), dtype(1)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + one)
        w = half * t
        t = half / t
        return np.array([(m[2, 1] - m[1, 2]) * t, (m[0, 2] - m[2, 0]) * t, (m[1, 0] - m[0, 1]) * t, w], dtype=dtype)
    i = 0
    if m[1, 1] > m[0, 0]:
        i = 1
    if m[2, 2] > m[i, i]:
        i = 2
    j, k = (i + 1) % 3, (i + 2) % 3
    t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + one)
    v = [None] * 3
    v[i] = half * t
    t = half / t
    w = (m[k, j] - m[j, k]) * t
    v[j] = (m[j, i] + m[i, j]) * t
    v[k] = (m[k, i] + m[i, k]) * t
    return np.array([v[0], v[1], v[2], w], dtype=dtype)


def _mv(R, v):
    return R[:, 0] * v[0] + R[:, 1] * v[1] + R[:, 2] * v[2]


def _mm(A, B):
    return A[:, 0:1] * B[0:1, :] + A[:, 1:2] * B[1:2, :] + A[:, 2:3] * B[2:3, :]


def state_row(P, R, V, dtype=np.float64):
    return np.concatenate([P, quat_from_R(R, dtype), V])


def recurrence(P, q, V, ba, bg, g_norm, rows, dtype=np.float64, wrong=None):
    """(state [10], trajectory [max(0, n - 1), 10]) of the start state carried through rows [n, 7] = dt acc gyr, in `dtype`.
    wrong: one of the mistakes tests/test_dead_reckon.py shows the parity inputs would catch."""
    c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)   # noqa: E731
    P, V, ba, bg, rows = c(P), c(V), c(ba), c(bg), c(rows).reshape(-1, 7)
    if wrong == "swap_biases":
        ba, bg = bg, ba
    half, two = dtype(0.5), dtype(2)
    g = np.array([0, 0, 0 if wrong == "no_g" else g_norm], dtype=np.float64).astype(dtype)
    R = quat_R(quat_normalized(c(q), dtype), dtype)
    if wrong == "R_transposed":
        R = R.T.copy()
    traj = []
    for i in range(1, len(rows)):
        dt, acc_0, gyr_0, acc_1, gyr_1 = rows[i, 0], rows[i - 1, 1:4], rows[i - 1, 4:7], rows[i, 1:4], rows[i, 4:7]
        un_acc_0 = _mv(R, acc_0 - ba) - g
        un_gyr = (gyr_1 - bg) if wrong == "gyr_end" else (gyr_0 + gyr_1) * half - bg
        th = un_gyr * dt
        R = _mm(R, quat_R([th[0] / two, th[1] / two, th[2] / two, dtype(1)], dtype))
        un_acc_1 = _mv(R, acc_1 - ba) - g
        un_acc = (un_acc_0 + un_acc_1) * half
        P = P + (V * dt + un_acc * (half * dt * dt))
        V = V + un_acc * dt
        traj.append(state_row(P, R, V, dtype))
    return state_row(P, R, V, dtype), (np.array(traj, dtype=dtype) if traj else np.zeros((0, 10), dtype=dtype))


def window_dead_reckon(w, samples, g_norm, from_frame=-1, write=False, dtype=np.float64, wrong=None):
    """DeadReckoned of one window at its state arrays through samples [n, 35]"""
    rows = np.asarray(samples, float).reshape(-1, 35)[:, ROW]
    n_steps = max(0, len(rows) - 1)
    zero = DeadReckoned(np.zeros(10), np.zeros((n_steps, 10)), n_steps, NO_FRAME)
    f = w.F - 1 if from_frame == -1 else from_frame
    if f >= w.F or (write and f + 1 >= w.F):
        return zero
    start = [w.pose[f, 0:3], w.pose[f, 3:7], w.speed_bias[f, 0:3], w.speed_bias[f, 3:6], w.speed_bias[f, 6:9]]
    read = np.concatenate([rows[:1, 1:].ravel(), rows[1:].ravel()]) if n_steps else np.zeros(0)   # (the first row's dt is not read)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        state, traj = recurrence(*start, g_norm, rows, dtype, wrong)
    if not (all(np.isfinite(a).all() for a in start) and np.isfinite(read).all() and np.isfinite(state.astype(float)).all()):
        return zero._replace(status=NUMERIC)
    return DeadReckoned(state.astype(np.float64), traj.astype(np.float64), n_steps, OK)


def state_errors(got, ref):
    """(|dP|inf / max(1, |P|inf), the same for V, |dR|inf on the rotation matrices of the two quaternions) of state rows [10]"""
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    eP = np.abs(got[0:3] - ref[0:3]).max() / max(1.0, np.abs(ref[0:3]).max())
    eV = np.abs(got[7:10] - ref[7:10]).max() / max(1.0, np.abs(ref[7:10]).max())
    eR = np.abs(quat_R(got[3:7]) - quat_R(ref[3:7])).max()
    return float(eP), float(eV), float(eR)


def state_error(got, ref):
    return max(state_errors(got, ref))


def rows_error(got, ref):
    """the largest state_error over rows [n, 10]"""
    assert np.shape(got) == np.shape(ref)
    return max([state_error(a, b) for a, b in zip(got, ref)], default=0.0)
