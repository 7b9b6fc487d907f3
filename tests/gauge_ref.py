"""Test helper: the definitions of vilo_batch_gauge_fix and vilo_batch_failure_detection (include/vilo_gpu.h) in numpy, written from the
header's text and Estimator::double2vector / failureDetection (estimator.cpp:903-1003, :1005-1052). Every product and sum is a numpy scalar
or elementwise operation in the order the formula writes it (no BLAS call, which may fuse), in a dtype of the caller's choice (FP64, or
numpy.longdouble for the floor). Nothing of the kernels under test. The quaternion and matrix helpers are tests/deadreckon_ref.py's."""
import collections

import numpy as np

from deadreckon_ref import _mm, _mv, quat_from_R, quat_normalized, quat_R

GAUGE_OK, GAUGE_NUMERIC = 0, 1
FAILURE_OK, FAILURE_NUMERIC = 0, 1
FEW_TRACKS, BIG_BA, BIG_BG, BIG_TRANSLATION, BIG_Z, BIG_ANGLE = 1, 2, 4, 8, 16, 32

# FP64 floors of the two definitions, as tests/test_gauge_fix.py::test_fp64_floor_measured prints them over every case of the GPU parity
# test: the larger of (a) every input moved by one unit in the last place and (b) the same formulas in numpy.longdouble, rounded at the end.
# Gauge-fix metric: |dP|inf / max(1, |P|inf), the same for V, |dR|inf on the rotation matrices of the returned quaternions (their sign
# does not enter), and |d yaw_diff_deg| / 180 on the windows where the singular branch is not taken (within a degree of the Euler
# singularity the yaw of R2ypr is not a function of its input to any precision, and the fix does not use it there). Failure-detection
# metric: |dv| / max(1, |v|) per compared quantity. Measured (x86-64): gauge fix (a) 1.4e-14 (b) 2.4e-15, yaw_diff_deg / 180 (a) 4.5e-15
# (b) 7.9e-16: the cases a degree or so off the Euler singularity carry it, where a unit in the last place of a quaternion moves the yaw by
# 1 / cos(pitch) ~ 50 of them; failure detection (a) 9.5e-16 (b) 1.9e-14, the acos of a quaternion's w near 1 (angles of a few degrees)
# being the term that carries it. Rounded up to one digit.
# The GPU tolerance is ten times the floor.
FLOOR = 2e-14
TOL = 10 * FLOOR
FLOOR_FAILURE = 2e-14
TOL_FAILURE = 10 * FLOOR_FAILURE

GaugeFixed = collections.namedtuple("GaugeFixed", "pose speed_bias ex_pose yaw_diff_deg singular status")
Failure = collections.namedtuple("Failure", "flags would_reboot status values")


def R2ypr_deg(R, dtype=np.float64):
    """Utility::R2ypr (utility.h:87-99), degrees"""
    n, o, a = R[:, 0], R[:, 1], R[:, 2]
    pi, d180 = dtype(np.pi), dtype(180)
    y = np.arctan2(n[1], n[0])
    p = np.arctan2(-n[2], n[0] * np.cos(y) + n[1] * np.sin(y))
    r = np.arctan2(a[0] * np.sin(y) - a[1] * np.cos(y), -o[0] * np.sin(y) + o[1] * np.cos(y))
    return np.array([y / pi * d180, p / pi * d180, r / pi * d180], dtype=dtype)


def gauge_fix(anchor, pose, speed_bias, ex_pose, ex_const=False, dtype=np.float64, wrong=None):
    """GaugeFixed of one window: anchor [7], pose [F, 7], speed_bias [F, 9], ex_pose [2, 7] -> the fixed arrays (FP64 copies; the inputs are
    not written). wrong: one of the mistakes tests/test_gauge_fix.py shows the parity inputs would catch."""
    c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)   # noqa: E731
    read = [np.asarray(anchor, float), np.asarray(pose, float), np.asarray(speed_bias, float)[:, :3]] + ([] if ex_const else [np.asarray(ex_pose, float)[:, 3:]])
    out_p, out_s, out_e = (np.array(a, dtype=np.float64) for a in (pose, speed_bias, ex_pose))
    if not all(np.isfinite(a).all() for a in read):
        return GaugeFixed(out_p, out_s, out_e, 0.0, 0, GAUGE_NUMERIC)
    anchor, pose, sb, ex = c(anchor), c(pose), c(speed_bias), c(ex_pose)
    if wrong == "anchor_solved":
        anchor = pose[0].copy()
    one, zero, d180, d90, pi = dtype(1), dtype(0), dtype(180), dtype(90), dtype(np.pi)
    Rs0, R00 = quat_R(anchor[3:7], dtype), quat_R(pose[0, 3:7], dtype)
    o0, o00 = R2ypr_deg(Rs0, dtype), R2ypr_deg(R00, dtype)
    y_diff = o0[0] - o00[0]
    yd = y_diff / d180 * pi
    rot = np.array([[np.cos(yd), -np.sin(yd), zero], [np.sin(yd), np.cos(yd), zero], [zero, zero, one]], dtype=dtype)
    singular = bool(abs(abs(o0[1]) - d90) < one or abs(abs(o00[1]) - d90) < one)
    if singular:
        rot = _mm(Rs0, R00.T.copy())
    P0, origin = pose[0, 0:3].copy(), anchor[0:3]
    for i in range(len(pose)):
        Ri = _mm(rot, quat_R(quat_normalized(pose[i, 3:7], dtype), dtype))
        Pi = _mv(rot, pose[i, 0:3] - P0) + origin
        Vi = sb[i, 0:3] if wrong == "no_velocity_rotation" else _mv(rot, sb[i, 0:3])
        out_p[i, 0:3], out_p[i, 3:7], out_s[i, 0:3] = Pi.astype(np.float64), quat_from_R(Ri, dtype).astype(np.float64), Vi.astype(np.float64)
    if not ex_const:
        for k in range(2):
            out_e[k, 3:7] = quat_from_R(quat_R(quat_normalized(ex[k, 3:7], dtype), dtype), dtype).astype(np.float64)
    return GaugeFixed(out_p, out_s, out_e, float(y_diff), int(singular), GAUGE_OK)


def window_gauge_fix(w, anchor=None, before=None, dtype=np.float64, wrong=None):
    """GaugeFixed of a window at its state arrays; anchor [7], or frame 0 of `before` (the state arrays before the solve)"""
    a = before[0][0] if anchor is None else anchor
    return gauge_fix(a, w.pose[:w.F], w.speed_bias[:w.F], w.ex_pose, bool(w.ex_const), dtype, wrong)


def failure_detection(pose_n, sb_n, last_track_num=None, last_pose=None, dtype=np.float64, wrong=None):
    """Failure of one window: pose_n [7] and sb_n [9] of its last frame, the caller's track count and last pose [7] (None: their bits 0)"""
    c = lambda a: np.asarray(a, dtype=np.float64).astype(dtype)   # noqa: E731
    read = [np.asarray(sb_n, float)[3:9]] + ([np.asarray(pose_n, float), np.asarray(last_pose, float)] if last_pose is not None else [])
    if not all(np.isfinite(a).all() for a in read):
        return Failure(0, 0, FAILURE_NUMERIC, np.zeros(6))
    sb = c(sb_n)
    Ba, Bg = (sb[6:9], sb[3:6]) if wrong == "swap_biases" else (sb[3:6], sb[6:9])
    v = [dtype(0)] * 6
    flags = 0
    if last_track_num is not None:
        v[0] = dtype(int(last_track_num))
        flags |= FEW_TRACKS if int(last_track_num) < 2 else 0
    v[1] = np.sqrt(Ba[0] * Ba[0] + Ba[1] * Ba[1] + Ba[2] * Ba[2])
    v[2] = np.sqrt(Bg[0] * Bg[0] + Bg[1] * Bg[1] + Bg[2] * Bg[2])
    flags |= BIG_BA if v[1] > dtype(2.5) else 0
    flags |= BIG_BG if v[2] > dtype(1.0) else 0
    if last_pose is not None:
        p, lp = c(pose_n), c(last_pose)
        d = p[0:3] - lp[0:3]
        v[3] = np.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
        v[4] = abs(p[2] - lp[2])
        delta_R = _mm(quat_R(quat_normalized(p[3:7], dtype), dtype).T.copy(), quat_R(quat_normalized(lp[3:7], dtype), dtype))
        with np.errstate(invalid="ignore"):
            # (3.14 is the reference's, :1045)
            v[5] = np.arccos(quat_from_R(delta_R, dtype)[3]) * dtype(2.0) / (dtype(np.pi) if wrong == "pi" else dtype(3.14)) * dtype(180.0)
        flags |= BIG_TRANSLATION if v[3] > dtype(5) else 0
        flags |= BIG_Z if v[4] > dtype(1) else 0
        flags |= BIG_ANGLE if v[5] > dtype(50) else 0
    return Failure(flags, int(bool(flags & (BIG_BA | BIG_BG))), FAILURE_OK, np.array([float(x) for x in v]))


THRESHOLDS = (2.0, 2.5, 1.0, 5.0, 1.0, 50.0)   # what values[k] is compared with, in bit order


def window_failure_detection(w, last_track_num=None, last_pose=None, dtype=np.float64, wrong=None):
    n = w.F - 1
    return failure_detection(w.pose[n], w.speed_bias[n], last_track_num, last_pose, dtype, wrong)


def gauge_errors(got, ref, F):
    """(|dP|inf / max(1, |P|inf), the same for V, |dR|inf over the frames' and the extrinsics' quaternions) of (pose, speed_bias, ex_pose)"""
    gp, gs, ge = (np.asarray(a, float) for a in got)
    rp, rs, re_ = (np.asarray(a, float) for a in ref)
    eP = np.abs(gp[:F, :3] - rp[:F, :3]).max() / max(1.0, np.abs(rp[:F, :3]).max())
    eV = np.abs(gs[:F, :3] - rs[:F, :3]).max() / max(1.0, np.abs(rs[:F, :3]).max())
    eR = max(np.abs(quat_R(a) - quat_R(b)).max() for a, b in list(zip(gp[:F, 3:7], rp[:F, 3:7])) + list(zip(ge[:, 3:7], re_[:, 3:7])))
    return float(eP), float(eV), float(eR)


def gauge_error(got, ref, F):
    return max(gauge_errors(got, ref, F))


def values_error(got, ref):
    got, ref = np.asarray(got, float), np.asarray(ref, float)
    return float((np.abs(got - ref) / np.maximum(1.0, np.abs(ref))).max())
