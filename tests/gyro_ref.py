"""Test helper (no test in it): the definition of vilo_batch_gyro_bias_align (include/vilo_gpu.h) in numpy, straight from
solveGyroscopeBias (src/initial/initial_aligment.cpp:14-40): per interval q_ij from the poses, the record's d(rotation)/d(gyro bias) block
and delta_q, r = 2 vec(gamma^-1 q_ij), A = sum J^T J, b = sum J^T r, the step from numpy.linalg.solve. A second route (numpy.linalg.lstsq on
the stacked J_k, r_k) measures the floor with tests/test_gyro_align.py, which also documents where FLOOR comes from."""
import collections

import numpy as np

OK, NO_INTERVALS, SINGULAR, NUMERIC = 0, 1, 2, 3   # VILO_GYRO_*

# FP64 floor of the step, |d delta_bg|_inf / max(1, |delta_bg|_inf), and of the two costs (relative), by DESIGN §4.13's rule: the larger
# of (a) every quaternion, delta_q and Jacobian entry moved by one unit in the last place and (b) solve against lstsq, over the packing
# shapes x use_leg x {initial, solved} x both linearizations (tests/test_gyro_align.py::test_fp64_floor_measured prints both: step
# (a) 1.5e-16 (b) 6.2e-17, costs (a) 1.8e-13). The step's tolerance is ten times its floor; the costs' bound of 1e-10 relative is the one
# the call was specified with, above ten times their floor.
FLOOR = 2e-16
FLOOR_COST = 2e-13
TOL = 10 * FLOOR
TOL_COST = 1e-10

# write-back and a second call of the corrected form: |second step| <= QUADRATIC_K |first step|^2 + TOL. The largest ratio
# |d2| / |d1|^2 of the definition over the cases of tests/test_gyro_align.py is 1.05 s/rad (the six-frame window at its solved state,
# |d1| = 4.7e-5: what is left there is the second-order term in the biases' whole distance from the records' point, not in d1 alone);
# the constant is that, doubled.
QUADRATIC_K = 2.0

# where a record keeps what the alignment reads (doubles): vilo_preint / vilo_preint_imu of include/vilo_gpu.h
_LEG = dict(dq=4, lin_bg=26, jac=33, n=31, col=24)    # (ILO_R, ILO_BG) = (3, 24), parameters.h:138,145
_IMU = dict(dq=4, lin_bg=14, jac=17, n=15, col=12)    # (O_R, O_BG) = (3, 12), parameters.h:121,124

Parts = collections.namedtuple("Parts", "q dq lin_bg J bg")
Alignment = collections.namedtuple("Alignment", "delta_bg initial_cost model_cost n_intervals status A b J r")


def qmul(a, b):
    """Hamilton product, quaternions as [x y z w]"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx,
                     aw * bz + ax * by - ay * bx + az * bw, aw * bw - ax * bx - ay * by - az * bz])


def qinv(a):
    return np.array([-a[0], -a[1], -a[2], a[3]]) / np.dot(a, a)


def delta_q(theta):
    """Utility::deltaQ (utility.h:28-41): not normalised"""
    return np.array([theta[0] / 2.0, theta[1] / 2.0, theta[2] / 2.0, 1.0])


def exp_q(theta):
    """the unit quaternion of the rotation vector theta"""
    a = np.linalg.norm(theta)
    s = 0.5 if a < 1e-12 else np.sin(a / 2.0) / a
    return np.array([theta[0] * s, theta[1] * s, theta[2] * s, np.cos(a / 2.0)])


def records(w):
    """(the window's record array, its layout) for the factor kind it uses"""
    return (w.preint, _LEG) if w.use_leg else (w.preint_imu, _IMU)


def parts(w, rec=None):
    """what the definition reads of window w at its state arrays: pose quaternions [F, 4] (as stored), and per interval delta_q [n, 4],
    lin_bg [n, 3], the Jacobian block [n, 3, 3]; the frames' gyro biases [F, 3]. rec: records to read instead of the window's own."""
    r0, lay = records(w)
    rec = r0 if rec is None else rec
    n = w.F - 1
    jac = rec[:n, lay["jac"]:lay["jac"] + lay["n"] ** 2].reshape(n, lay["n"], lay["n"])
    return Parts(w.pose[:w.F, 3:7].copy(), rec[:n, lay["dq"]:lay["dq"] + 4].copy(), rec[:n, lay["lin_bg"]:lay["lin_bg"] + 3].copy(),
                 jac[:, 3:6, lay["col"]:lay["col"] + 3].copy(), w.speed_bias[:w.F, 6:9].copy())


def rows(p, linearization="record"):
    """(J [n, 3, 3], r [n, 3]) of the intervals"""
    n = p.dq.shape[0]
    r = np.zeros((n, 3))
    for k in range(n):
        qi, qj = p.q[k] / np.linalg.norm(p.q[k]), p.q[k + 1] / np.linalg.norm(p.q[k + 1])
        g = p.dq[k]
        if linearization == "corrected":
            g = qmul(g, delta_q(p.J[k] @ (p.bg[k] - p.lin_bg[k])))
        else:
            assert linearization == "record"
        e = qmul(qinv(g), qmul(qinv(qi), qj))
        r[k] = (-2.0 if e[3] < 0.0 else 2.0) * e[:3]   # (w >= 0, as the quaternion of R_k^T R_{k+1} has it in the reference)
    return p.J, r


def _finish(J, r, d, status):
    n = J.shape[0]
    A = np.einsum("kij,kil->jl", J, J)
    b = np.einsum("kij,ki->j", J, r)
    ic = 0.5 * float((r * r).sum())
    e = r - np.einsum("kij,j->ki", J, d)
    return Alignment(d, ic, 0.5 * float((e * e).sum()) if status == OK else ic, n, status, A, b, J, r)


def align_parts(p, linearization="record"):
    J, r = rows(p, linearization)
    n = J.shape[0]
    zero = np.zeros(3)
    if n < 1:
        return Alignment(zero, 0.0, 0.0, 0, NO_INTERVALS, np.zeros((3, 3)), zero, J, r)
    A = np.einsum("kij,kil->jl", J, J)
    b = np.einsum("kij,ki->j", J, r)
    if not (np.isfinite(A).all() and np.isfinite(b).all() and np.isfinite(r).all()):
        return _finish(J, r, zero, NUMERIC)
    try:
        np.linalg.cholesky(A)   # (the call's LDL^T has three positive pivots exactly when A is positive definite)
    except np.linalg.LinAlgError:
        return _finish(J, r, zero, SINGULAR)
    return _finish(J, r, np.linalg.solve(A, b), OK)


def align(w, linearization="record", rec=None):
    """the definition at window w's state arrays"""
    return align_parts(parts(w, rec), linearization)


def align_lstsq(p, linearization="record"):
    """the second route: least squares on the stacked rows (no normal equations)"""
    J, r = rows(p, linearization)
    return np.linalg.lstsq(J.reshape(-1, 3), r.reshape(-1), rcond=None)[0]


def step_error(d, ref):
    return float(np.abs(np.asarray(d) - ref).max() / max(1.0, np.abs(ref).max()))


def with_gyro_bias(w, d):
    """a twin of w with d added to every frame's gyro bias (what write = 1 does)"""
    t = w.twin()
    t.speed_bias[:w.F, 6:9] = w.speed_bias[:w.F, 6:9] + d
    return t


def propagated(w):
    """a twin of w whose rotations are chained from its own records, q_{k+1} = q_k (x) delta_q_k, and whose gyro biases are the records'
    linearisation points (the last frame takes the last interval's): the window manager's IMU-propagated start-up poses"""
    t = w.twin()
    p = parts(w)
    q = t.pose[0, 3:7] / np.linalg.norm(t.pose[0, 3:7])
    t.pose[0, 3:7] = q
    for k in range(w.F - 1):
        q = qmul(q, p.dq[k])
        q = q / np.linalg.norm(q)
        t.pose[k + 1, 3:7] = q
    t.speed_bias[:w.F - 1, 6:9] = p.lin_bg
    t.speed_bias[w.F - 1, 6:9] = p.lin_bg[-1]
    return t


def with_rotated_records(w, d):
    """a twin of w with records of its own in which every interval's delta_q is rotated by Exp(-J_k d): the records of a gyro whose bias
    is d away, to first order. The alignment of propagated(w) on these records returns d up to the second-order term."""
    t = w.twin()
    rec, lay = records(w)
    rec = rec.copy()
    p = parts(w)
    for k in range(w.F - 1):
        g = qmul(p.dq[k], exp_q(-(p.J[k] @ d)))
        rec[k, lay["dq"]:lay["dq"] + 4] = g
    if w.use_leg:
        t.preint = rec
    else:
        t.preint_imu = rec
    return t
