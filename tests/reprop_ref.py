"""Test helper: the point, drift, selection and status logic of vilo_batch_repropagate (include/vilo_gpu.h) in numpy, written from the
header's text and the reference's start-up loop (estimator.cpp:752-760). Every product and sum is a numpy scalar operation in the order
the header writes it, in a dtype of the caller's choice (FP64, or numpy.longdouble for the floor). Nothing of the kernels under test; the
integration itself is not restated here (the GPU tests compare it with vilo_preintegrate bit for bit and with the oracle)."""
import collections
import functools

import numpy as np

OK, NOT_SELECTED, NO_INTERVAL, NO_SAMPLES, NUMERIC = 0, 1, 2, 3, 4
POINTS, SELECTS = ("state", "startup", "given"), ("all", "drifted", "mask")

# FP64 floor of the drifts, as tests/test_repropagate.py::test_fp64_floor_measured prints it over every case of cases(): the larger of
# (a) every input (state biases, record's lin_*, the caller's rows) moved by one unit in the last place and (b) the same formulas in
# numpy.longdouble, rounded at the end. Metric: |d drift| / max(1, |point|inf, |lin|inf). Measured (x86-64): (a) 1.1e-16 (b) 1.4e-17:
# a difference of two numbers below 1 and a norm of three or four such. Rounded up to one digit. The GPU tolerance is ten times the
# floor.
FLOOR = 2e-16
TOL = 10 * FLOOR

# tests/test_repropagate.py::test_startup_sequence_ratio_of_the_oracle: every gyro bias of case window "F11" moved by STARTUP_OFFSET,
# gyro_bias_align (record form, written back), every record integrated again by the oracle at (0, Bg_{k+1}, rho_{k+1}), gyro_bias_align
# again: |second delta_bg| / |first delta_bg| (2-norms). The CPU test recomputes it and holds it to 1 % of this figure; the GPU test
# gates its own ratio at ten times it.
STARTUP_OFFSET = (4e-3, -3e-3, 2e-3)
STARTUP_RATIO = 0.144223   # |d1| 3.617e-2 rad/s (the synthetic poses' noise carries it), |d2| 5.217e-3 rad/s

# thresholds of the DRIFTED cases: between the drifts the case windows have (test_drifted_cases_are_clear_of_their_thresholds holds every
# drift at least 1e-6 relative away from its threshold, so that no rounding flips a selection)
THRESHOLDS = (0.035, 0.0035, 0.0040)

Result = collections.namedtuple("Result", "drift selected status rows")


def record_lin(w):
    """[10, 10] lin_ba lin_bg lin_rho of the window's records as the batch reads them (use_leg == 0: the IMU records, rho 0)"""
    out = np.zeros((10, 10))
    n = w.F - 1
    if w.use_leg:
        out[:n] = w.preint[:n, 23:33]
    else:
        out[:n, :6] = w.preint_imu[:n, 11:17]
    return out


def evaluate(w, rec_lin, point="state", select="all", write=True, lin=None, mask=None, thresholds=(0.10, 0.01, 0.01), counts=None,
             dtype=np.float64):
    """the ten intervals of window w at its state arrays: Result(drift [10, 3], selected [10], status [10], rows [10, 10] = the point of
    every interval that has one). rec_lin [10, 10]: the records' own point; counts [10]: samples per interval (write)."""
    leg = bool(w.use_leg)
    nl = 10 if leg else 6
    sb, lb, rl = w.speed_bias.astype(dtype), w.leg_bias.astype(dtype), np.asarray(rec_lin).astype(dtype)
    th = [dtype(t) for t in thresholds]
    drift, selected, status, rows = np.zeros((10, 3), dtype), np.zeros(10, np.int32), np.full(10, NO_INTERVAL, np.int32), np.zeros((10, 10), dtype)
    for k in range(10):
        if k >= w.F - 1:
            continue
        p = np.zeros(10, dtype)
        if point == "given":
            p[:nl] = np.asarray(lin, dtype=np.float64).reshape(10, 10)[k, :nl].astype(dtype)
        else:
            fr = k + 1 if point == "startup" else k
            if point == "state":
                p[0:3] = sb[fr, 3:6]
            p[3:6] = sb[fr, 6:9]
            if leg:
                p[6:10] = lb[fr]
        rows[k] = p
        if not np.isfinite(p.astype(np.float64)).all():
            status[k] = NUMERIC
            continue
        d = np.zeros(10, dtype)
        d[:nl] = p[:nl] - rl[k, :nl]
        drift[k, 0] = np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])
        drift[k, 1] = np.sqrt((d[3] * d[3] + d[4] * d[4]) + d[5] * d[5])
        drift[k, 2] = np.sqrt(((d[6] * d[6] + d[7] * d[7]) + d[8] * d[8]) + d[9] * d[9])
        if select == "all":
            selected[k] = 1
        elif select == "mask":
            selected[k] = 1 if np.asarray(mask).reshape(10)[k] else 0
        else:
            selected[k] = 0 if (drift[k, 0] <= th[0] and drift[k, 1] <= th[1] and drift[k, 2] <= th[2]) else 1
        if not selected[k]:
            status[k] = NOT_SELECTED
        elif write and counts is not None and counts[k] < 2:
            status[k] = NO_SAMPLES
        else:
            status[k] = OK
    return Result(drift, selected, status, rows)


def spread_biases(w, seed):
    """w with every frame's biases moved by amounts of its own (2e-2 m/s^2, 2e-3 rad/s, 2e-3 m, normal): the state's biases leave the
    records' point, and neighbouring frames differ, so that the start frame's biases are not the end frame's"""
    rng = np.random.default_rng(seed)
    w.speed_bias[:, 3:6] += 2e-2 * rng.normal(size=(11, 3))
    w.speed_bias[:, 6:9] += 2e-3 * rng.normal(size=(11, 3))
    w.leg_bias += 2e-3 * rng.normal(size=(11, 4))
    return w


@functools.lru_cache(maxsize=None)
def case_window(name):
    """tests/test_gauge_fix.py's packing shapes (11, 6 and 2 frames with use_leg = 1, an IMU-only window of 11) with spread biases; the
    synthetic generator's own samples (a few dozen per interval)"""
    from test_gauge_fix import shape_window
    w = shape_window(name).twin()
    w.preint, w.preint_imu = w.preint.copy(), w.preint_imu.copy()
    return spread_biases(w, {"F11": 1, "F6": 2, "F2": 3, "F11imu": 4}[name])


LEG_CASES, IMU_CASES = ("F11", "F6", "F2"), ("F11imu",)


def counts(w):
    return np.diff(np.asarray(w.sample_offsets, dtype=np.int64))


def given_rows(w, seed=9):
    """[10, 10] rows of a caller's own: the records' point moved by amounts of the drifts' size"""
    rng = np.random.default_rng(seed)
    return record_lin(w) + rng.normal(size=(10, 10)) * np.array([3e-2] * 3 + [3e-3] * 3 + [3e-3] * 4)


def mask_of(w, seed=5):
    m = (np.random.default_rng(seed).random(10) < 0.5).astype(np.uint8)
    m[0], m[min(1, w.F - 2)] = 1, 0 if w.F > 2 else 1
    return m


def cases():
    """(tag, window, kwargs of evaluate) of every CPU / GPU parity case"""
    out = []
    for name in LEG_CASES + IMU_CASES:
        w = case_window(name)
        for point in POINTS:
            for select in SELECTS:
                kw = dict(point=point, select=select, thresholds=THRESHOLDS)
                if point == "given":
                    kw["lin"] = given_rows(w)
                if select == "mask":
                    kw["mask"] = mask_of(w)
                out.append(("%s %s %s" % (name, point, select), w, kw))
    return out
