"""CPU: the numpy definition of vilo_batch_repropagate's point, drift, selection and status logic (tests/reprop_ref.py): reprop_opts'
argument checks, the measured FP64 floor of the drifts, the clearance of the DRIFTED cases from their thresholds, every status, the
start-up point against the start frame's biases in units of the GPU parity bounds, and the oracle's ratio of the start-up sequence."""
import numpy as np
import pytest

import reprop_ref as R


def test_python_surface_exists():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    import ctypes as C
    assert callable(api.Batch.repropagate) and callable(api.Context.window_repropagate)
    assert C.sizeof(T.RepropOpts) == 40 and C.sizeof(T.IntervalRepropRecord) == 32
    assert (T.REPROP_OK, T.REPROP_NOT_SELECTED, T.REPROP_NO_INTERVAL, T.REPROP_NO_SAMPLES, T.REPROP_NUMERIC) == (R.OK, R.NOT_SELECTED, R.NO_INTERVAL, R.NO_SAMPLES, R.NUMERIC)


def test_reprop_opts_checks():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    o, lin, mask = api.reprop_opts()
    assert (o.point, o.select, o.write) == (0, 0, 1) and lin is None and mask is None
    assert (o.ba_threshold, o.bg_threshold, o.rho_threshold) == T.REPROP_THRESHOLDS == (0.10, 0.01, 0.01)
    o, lin, mask = api.reprop_opts("given", "mask", False, lin=np.zeros((2, 10, 10)), mask=np.ones((2, 10)), thresholds=(1, 2, 3), n_windows=2)
    assert (o.point, o.select, o.write) == (2, 2, 0) and lin.shape == (20, 10) and mask.shape == (20,) and mask.dtype == np.uint8
    assert (o.ba_threshold, o.bg_threshold, o.rho_threshold) == (1.0, 2.0, 3.0)
    for kw in (dict(point="frame"), dict(select="some"), dict(point="given"), dict(lin=np.zeros((10, 10))), dict(select="mask"),
               dict(mask=np.zeros(10)), dict(thresholds=(0.1, 0.1)), dict(thresholds=(0.1, -1e-9, 0.1)), dict(thresholds=(0.1, np.nan, 0.1)),
               dict(thresholds=(np.inf, 0.1, 0.1)), dict(point="given", lin=np.zeros((10, 9))), dict(point="given", lin=np.zeros((10, 10)), n_windows=2),
               dict(select="mask", mask=np.zeros(7)), dict(select="mask", mask=np.zeros(10), n_windows=2)):
        with pytest.raises(ValueError):
            api.reprop_opts(**kw)


def test_fp64_floor_measured():
    fa = fb = 0.0
    rng = np.random.default_rng(3)
    ud = lambda a: np.nextafter(a, rng.choice([-np.inf, np.inf], a.shape))
    for tag, w, kw in R.cases():
        rl = R.record_lin(w)
        ref = R.evaluate(w, rl, **kw)
        hi = R.evaluate(w, rl, dtype=np.longdouble, **kw)
        scale = max(1.0, np.abs(ref.rows).max(), np.abs(rl).max())
        fb = max(fb, float(np.abs(hi.drift.astype(np.float64) - ref.drift).max()) / scale)
        assert (hi.selected == ref.selected).all() and (hi.status == ref.status).all(), tag
        for _ in range(8):
            t = w.twin()
            t.speed_bias, t.leg_bias = ud(w.speed_bias), ud(w.leg_bias)
            kw2 = dict(kw, lin=ud(kw["lin"])) if "lin" in kw else kw
            m = R.evaluate(t, ud(rl), **kw2)
            fa = max(fa, float(np.abs(m.drift - ref.drift).max()) / scale)
            assert (m.selected == ref.selected).all() and (m.status == ref.status).all(), tag
    print("MEASURED drift floor: (a) one unit in the last place %.1e, (b) longdouble %.1e; FLOOR %.0e, TOL %.0e" % (fa, fb, R.FLOOR, R.TOL))
    assert max(fa, fb) <= R.FLOOR and R.FLOOR <= 4 * max(fa, fb) and R.TOL == 10 * R.FLOOR


def test_drifted_cases_are_clear_of_their_thresholds_and_every_outcome_occurs():
    clear, seen_sel, seen_status = np.inf, set(), set()
    for tag, w, kw in R.cases():
        ref = R.evaluate(w, R.record_lin(w), counts=R.counts(w), **kw)
        n = w.F - 1
        seen_sel |= set(ref.selected[:n].tolist())
        seen_status |= set(ref.status.tolist())
        assert (ref.status[n:] == R.NO_INTERVAL).all() and not ref.drift[n:].any() and not ref.selected[n:].any()
        if kw["select"] == "drifted":
            c = np.abs(ref.drift[:n] / np.array(R.THRESHOLDS) - 1.0)[:, :3 if w.use_leg else 2]
            clear = min(clear, float(c.min()))
    print("MEASURED smallest relative distance of a drift from its threshold: %.1e" % clear)
    assert clear >= 1e-6
    # one sample in interval 3 (write only), a NaN gyro bias in frame 4 (state: interval 4; startup: interval 3)
    w = R.case_window("F11").twin()
    cnt = R.counts(w).copy()
    cnt[3] = 1
    w.speed_bias[4, 7] = np.nan
    a = R.evaluate(w, R.record_lin(w), counts=cnt)
    assert a.status[3] == R.NO_SAMPLES and a.selected[3] == 1 and a.status[4] == R.NUMERIC and a.selected[4] == 0 and not a.drift[4].any()
    assert R.evaluate(w, R.record_lin(w), write=False, counts=cnt).status[3] == R.OK
    b = R.evaluate(w, R.record_lin(w), point="startup", counts=cnt)
    assert b.status[3] == R.NUMERIC and b.status[4] == R.OK
    seen_status |= set(a.status.tolist())
    assert seen_sel == {0, 1} and seen_status == {R.OK, R.NOT_SELECTED, R.NO_INTERVAL, R.NO_SAMPLES, R.NUMERIC}
    # a record whose own point is no number is selected by DRIFTED; IMU-only intervals have no rho drift
    rl = R.record_lin(w)
    rl[0, 4] = np.nan
    assert R.evaluate(w, rl, select="drifted", thresholds=(10, 10, 10)).selected[0] == 1
    wi = R.case_window("F11imu")
    assert not R.evaluate(wi, R.record_lin(wi)).drift[:, 2].any()


def test_startup_point_is_the_end_frames(ocfg):
    """interval k at (0, Bg_{k+1}, rho_{k+1}): with the start frame's biases instead, the oracle's records move by at least 1000 times
    the bounds the GPU parity test applies (state entries: rtol 1e-12, atol 1e-14, tests/test_gpu_parity.py::test_preintegrate)"""
    from oracle import oracle_py as O
    for name in R.LEG_CASES:
        w = R.case_window(name)
        rows = R.evaluate(w, R.record_lin(w), point="startup").rows
        worst = np.inf
        for k in range(w.F - 1):
            a, b = w.sample_offsets[k], w.sample_offsets[k + 1]
            np.testing.assert_array_equal(rows[k], np.concatenate([np.zeros(3), w.speed_bias[k + 1, 6:9], w.leg_bias[k + 1]]))
            good = O.preintegrate_imu_leg(ocfg, w.samples[a:b], rows[k])
            bad = O.preintegrate_imu_leg(ocfg, w.samples[a:b], np.concatenate([np.zeros(3), w.speed_bias[k, 6:9], w.leg_bias[k]]))
            worst = min(worst, float((np.abs(good[:33] - bad[:33]) / (1e-12 * np.abs(good[:33]) + 1e-14)).max()))
        print("MEASURED %s: the start frame's biases move a record's state entries by at least %.1e bounds" % (name, worst))
        assert worst >= 1000.0


def startup_sequence_oracle(ocfg):
    """|second delta_bg| / |first delta_bg| of the start-up sequence with the oracle's repropagate (reprop_ref.STARTUP_RATIO)"""
    import gyro_ref
    from oracle import oracle_py as O
    w = R.case_window("F11").twin()
    w.speed_bias[:, 6:9] += np.array(R.STARTUP_OFFSET)
    d1 = gyro_ref.align(w, "record")
    t = gyro_ref.with_gyro_bias(w, d1.delta_bg)
    rows = R.evaluate(t, R.record_lin(t), point="startup").rows
    rec = np.zeros_like(w.preint)
    for k in range(10):
        a, b = w.sample_offsets[k], w.sample_offsets[k + 1]
        rec[k] = O.repropagate_imu_leg(ocfg, w.samples[a:b], w.lin[k], [rows[k]])[1]
    d2 = gyro_ref.align(t, "record", rec)
    return float(np.linalg.norm(d2.delta_bg) / np.linalg.norm(d1.delta_bg))


def test_startup_sequence_ratio_of_the_oracle(ocfg):
    ratio = startup_sequence_oracle(ocfg)
    print("MEASURED start-up sequence, oracle: |d2| / |d1| = %.6e (stored %.6e)" % (ratio, R.STARTUP_RATIO))
    assert abs(ratio - R.STARTUP_RATIO) <= 0.01 * R.STARTUP_RATIO
