"""GPU (-m gpu): vilo_batch_gyro_bias_align / vilo_window_gyro_bias_align against the numpy definition (tests/gyro_ref.py) at the state the
device returns: parity on the packing shapes for both factor kinds and both linearizations, a field window, an interval above 10 s,
independence of batch size and position across the kernel's seams, freedom from side effects, the write-back and what follows it (reset,
solve, graph replay, the quadratic bound of a second call), a singular and a non-finite window, negated quaternions, samples in force, the host form, the call's device memory, bad arguments. Tolerance: ten times
the FP64 floor tests/test_gyro_align.py measures (gyro_ref.TOL); costs within gyro_ref.TOL_COST = 1e-10 relative."""
import ctypes as C

import numpy as np
import pytest

import gyro_ref
from test_covariance_gpu import _window
from test_gyro_align import kind_window
from test_triangulate import SHAPES, shape_window

pytestmark = pytest.mark.gpu

OK, NONE, SINGULAR, NUMERIC = gyro_ref.OK, gyro_ref.NO_INTERVALS, gyro_ref.SINGULAR, gyro_ref.NUMERIC
LINS = ("record", "corrected")


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _row(r, i):
    return [np.ascontiguousarray(r.delta_bg[i])] + [np.asarray(x[i]) for x in r[1:]]


def _bitwise(x, y):
    for a, b in zip(x, y):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert a.tobytes() == b.tobytes()


def _state(ws):
    return [a.copy() for w in ws for a in w.state_arrays()]


def _two_frames(use_leg):
    """the first two frames of the 70-landmark window: one interval, the smallest window a batch accepts"""
    from test_gpu_parity import _truncate
    w = kind_window("L70", use_leg).twin()
    w.prior = w.prior.copy()   # (_truncate switches the prior off in place: not the cached window's)
    _truncate(w, 2)
    return w


def _check_parity(r, i, w, tag, lin, rec=None, tol=gyro_ref.TOL):
    """window i of the report against the definition at w's state arrays; returns the step's error"""
    ref = gyro_ref.align(w, lin, rec)
    assert ref.status == OK, tag
    assert r.status[i] == OK and r.n_intervals[i] == w.F - 1 == ref.n_intervals, (tag, r.status[i], r.n_intervals[i])
    e = gyro_ref.step_error(r.delta_bg[i], ref.delta_bg)
    ei = abs(r.initial_cost[i] - ref.initial_cost) / ref.initial_cost
    em = abs(r.model_cost[i] - ref.model_cost) / ref.model_cost if ref.model_cost > 0.0 else 0.0
    print("MEASURED %s %s: step %.1e (tolerance %.0e), initial_cost %.1e, model_cost %.1e (bound %.0e); |delta_bg| %.1e"
          % (tag, lin, e, tol, ei, em, gyro_ref.TOL_COST, np.abs(ref.delta_bg).max()))
    assert e <= tol, (tag, lin, e)
    assert ei <= gyro_ref.TOL_COST, (tag, lin, ei)
    if ref.n_intervals == 1:
        # one interval: J is square and invertible, the fit is exact and model_cost is the rounding of zero on either side, to which no
        # relative bound applies. r - J delta_bg is then a few units in the last place of r (cond(J) is 1: J is close to -sum_dt I):
        # |r - J delta_bg| <= 1e-14 |r|, 45 such units, i.e. model_cost <= 1e-28 initial_cost
        assert r.model_cost[i] <= 1e-28 * ref.initial_cost and ref.model_cost <= 1e-28 * ref.initial_cost, (tag, lin, r.model_cost[i], ref.model_cost)
    else:
        assert em <= gyro_ref.TOL_COST, (tag, lin, em)
    assert r.model_cost[i] <= r.initial_cost[i]
    return e


@pytest.mark.parametrize("use_leg", [1, 0])
@pytest.mark.parametrize("shape", sorted(SHAPES) + ["F2"])
def test_parity_with_numpy(ctx, shape, use_leg):
    """11 frames (L9, L70, L456), 6 (F6) and 2 (F2, at its initial state: two frames without a prior are no problem to solve); the
    initial state and the state after a 4-iteration solve, where the biases have left the records' linearisation point and the two
    linearizations differ."""
    from cerberus_amd import api
    w = _two_frames(use_leg) if shape == "F2" else kind_window(shape, use_leg).twin()
    ws = [w, w.twin()]
    ws[1].speed_bias[:w.F, 6:9] += 1e-3 * np.array([1.0, -2.0, 0.5])   # the same window with its biases away from the records' point
    b = api.Batch(ctx, ws)
    worst = 0.0
    for state in ("initial", "solved"):
        if state == "solved":
            if shape == "F2":
                break
            b.solve(api.default_solve_opts(True, 4))
            b.download()
        rs = {lin: b.gyro_bias_align(lin) for lin in LINS}
        for lin in LINS:
            for i in range(2):
                worst = max(worst, _check_parity(rs[lin], i, ws[i], "%s use_leg %d %s window %d" % (shape, use_leg, state, i), lin))
        assert rs["record"].delta_bg[1].tobytes() != rs["corrected"].delta_bg[1].tobytes()
    print("MEASURED %s use_leg %d: largest step error %.1e" % (shape, use_leg, worst))


def test_one_frame_is_refused_by_the_batch(ctx):
    """NO_INTERVALS needs n_frames < 2, which vilo_batch_create refuses: the status cannot be reached through a batch"""
    from cerberus_amd import api
    from test_landmark_covariance_gpu import _no_landmarks
    w = _no_landmarks(_two_frames(1))
    w.F = 1
    with pytest.raises(api.ViloError):
        api.Batch(ctx, [w])


def test_field_windows_and_a_long_interval(ctx, cfg, ocfg):
    from cerberus_amd import api
    import field_windows
    ws = [field_windows.field_window(cfg, ocfg, n) for n in ("f200", "f60_partial8")]
    b = api.Batch(ctx, ws)
    for state in ("initial", "solved"):
        if state == "solved":
            b.solve(api.default_solve_opts(True, field_windows.ITERS))
            b.download()
        for lin in LINS:
            r = b.gyro_bias_align(lin)
            for i, name in enumerate(("f200", "f60_partial8")):
                _check_parity(r, i, ws[i], "field %s %s" % (name, state), lin)
    # an interval of sum_dt > 10 s carries no factor and is counted all the same: nothing but its sum_dt differs, so nothing at all differs
    w = shape_window("L70")
    long_w = w.twin()
    long_w.preint = w.preint.copy()
    long_w.preint[4, 0] = 11.0
    r = api.Batch(ctx, [long_w, w.twin()]).gyro_bias_align()
    assert list(r.n_intervals) == [10, 10] and list(r.status) == [OK, OK]
    _check_parity(r, 0, long_w, "interval 4 above 10 s", "record")
    _bitwise(_row(r, 0), _row(r, 1))


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg):
    """1, 5 (a partial wave), 17 (a second workgroup) and 300 mixed shapes: every window bitwise what it is alone, wherever it sits"""
    from cerberus_amd import api
    bases = [shape_window("L9"), shape_window("F6"), _window(cfg, ocfg, seed=78, L=30), shape_window("L70"), _two_frames(1)]
    for lin in LINS:
        alone = [_row(api.Batch(ctx, [w.twin()]).gyro_bias_align(lin), 0) for w in bases]
        assert all(a[4] == OK for a in alone)
        assert len({a[0].tobytes() for a in alone}) == len(bases)
        for n, shift in ((5, 0), (5, 2), (17, 0), (17, 3), (300, 1)):
            ws = [bases[(i + shift) % len(bases)].twin() for i in range(n)]
            r = api.Batch(ctx, ws).gyro_bias_align(lin)
            for i in range(n):
                _bitwise(_row(r, i), alone[(i + shift) % len(bases)])


def _sequence(ctx, base, opts, report, samples=False):
    from cerberus_amd import api
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    if samples:
        b.set_samples()
    b.solve(opts)
    summ0 = b.download()
    before = _state(ws)
    out = None
    if report:
        out = [b.gyro_bias_align(lin) for lin in LINS]
        summ1 = b.download()
        for x, y in zip(before, _state(ws)):
            assert x.tobytes() == y.tobytes()
        assert [bytes(s) for s in summ0] == [bytes(s) for s in summ1]
    recs = [b.fetch(13, i).tobytes() for i in range(len(ws))]
    rr = b.residuals()
    res = [np.asarray(x).tobytes() for x in rr if x is not None]
    b.solve(opts)
    summ = b.download()
    return _state(ws), [bytes(s) for s in summ], res, recs, out, ws


def test_no_side_effects(ctx, cfg, ocfg):
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s, L=60) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)
    st_a, su_a, re_a, rc_a = _sequence(ctx, base, opts, False)[:4]
    st_b, su_b, re_b, rc_b = _sequence(ctx, base, opts, True)[:4]
    for x, y in zip(st_a, st_b):
        assert x.tobytes() == y.tobytes()
    assert su_a == su_b and re_a == re_b and rc_a == rc_b


def _singular(w):
    """the window with the rotation / gyro-bias block of every record's Jacobian zeroed"""
    t = w.twin()
    t.preint = w.preint.copy()
    jac = t.preint[:, 33:33 + 961].reshape(-1, 31, 31)
    jac[:, 3:6, 24:27] = 0.0
    return t


@pytest.mark.parametrize("replay", [False, True])
def test_write_back(ctx, replay):
    from cerberus_amd import api
    opts = api.default_solve_opts(True, 4)
    base = [shape_window("L70").twin(), _singular(shape_window("L9")), shape_window("F6").twin()]
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    if replay:
        b.solve(opts)   # solve once before the write: the solve after it replays the captured graph
        b.reset()
    b.download()
    before = _state(ws)
    dry = b.gyro_bias_align("corrected")
    r = b.gyro_bias_align("corrected", write=True)
    assert list(r.status) == [OK, SINGULAR, OK]
    for i in range(3):
        _bitwise(_row(r, i), _row(dry, i))
    assert not r.delta_bg[1].any() and r.model_cost[1] == r.initial_cost[1] > 0.0 and r.n_intervals[1] == 10
    b.download()
    after = _state(ws)
    for i, w in enumerate(ws):
        for j in range(6):
            x, y = after[6 * i + j], before[6 * i + j].copy()
            if j == 1 and r.status[i] == OK:   # speed_bias: the gyro bias of every frame of the window moved by exactly delta_bg
                y[:w.F, 6:9] = y[:w.F, 6:9] + r.delta_bg[i]
                assert x.tobytes() != before[6 * i + j].tobytes()
            assert x.tobytes() == y.tobytes(), (i, j)
    # the corrected form sees the written biases: the next step is within the quadratic bound of the definition (gyro_ref.QUADRATIC_K,
    # measured and fixed in tests/test_gyro_align.py); the record form does not see them and returns its first step again
    rec_first = api.Batch(ctx, [w.twin() for w in base]).gyro_bias_align("record")
    second, rec_second = b.gyro_bias_align("corrected"), b.gyro_bias_align("record")
    for i in (0, 2):
        n1, n2 = np.linalg.norm(r.delta_bg[i]), np.linalg.norm(second.delta_bg[i])
        _check_parity(second, i, ws[i], "after the write, window %d" % i, "corrected")
        print("MEASURED after the write, window %d: |d1| %.2e |d2| %.2e, |d2| / |d1|^2 %.2e (K = %.1f)" % (i, n1, n2, n2 / n1 ** 2, gyro_ref.QUADRATIC_K))
        assert n2 <= gyro_ref.QUADRATIC_K * n1 ** 2 + gyro_ref.TOL, (i, n1, n2)
        assert rec_second.delta_bg[i].tobytes() == rec_first.delta_bg[i].tobytes()
    # the solve after it starts from the new biases: a fresh batch created at that state gives the same, to the solver forms' own tolerance
    fresh = [w.twin() for w in ws]
    b.solve(opts)
    assert b.path()["replay"] == replay
    b.download()
    fb = api.Batch(ctx, fresh)
    fb.solve(opts)
    fb.download()
    for w, f in zip(ws, fresh):
        for x, y in zip(w.state_arrays(), f.state_arrays()):
            np.testing.assert_allclose(x, y, rtol=0, atol=1e-8)
    # the uploaded initial state is still what reset restores
    b.reset()
    b.download()
    for w, o in zip(ws, base):
        for x, y in zip(w.state_arrays(), o.state_arrays()):
            assert x.tobytes() == y.tobytes()


def test_corrected_form_converges_from_a_solved_state(ctx):
    """after a solve the steps are small (1e-4 .. 3e-3 rad/s on these windows), where gyro_ref.QUADRATIC_K |d1|^2 is far below any
    first-order error of the correction: write-back, second call"""
    from cerberus_amd import api
    ws = [kind_window(n, 0).twin() for n in ("L9", "L70", "L456", "F6")]
    b = api.Batch(ctx, ws)
    b.solve(api.default_solve_opts(True, 4))
    first = b.gyro_bias_align("corrected", write=True)
    second = b.gyro_bias_align("corrected")
    assert list(first.status) == [OK] * 4 and list(second.status) == [OK] * 4
    for i in range(4):
        n1, n2 = np.linalg.norm(first.delta_bg[i]), np.linalg.norm(second.delta_bg[i])
        print("MEASURED solved window %d: |d1| %.2e |d2| %.2e, |d2| / |d1|^2 %.2e (K = %.1f)" % (i, n1, n2, n2 / n1 ** 2, gyro_ref.QUADRATIC_K))
        assert n1 < 1e-2 and n2 <= gyro_ref.QUADRATIC_K * n1 ** 2 + gyro_ref.TOL, (i, n1, n2)


def test_pose_quaternions_of_either_hemisphere(ctx):
    """negated pose quaternions (the same rotations) change no bit"""
    from cerberus_amd import api
    w = shape_window("L70")
    t = w.twin()
    t.pose[1:w.F:2, 3:7] *= -1.0
    for lin in LINS:
        r = api.Batch(ctx, [w.twin(), t]).gyro_bias_align(lin)
        assert list(r.status) == [OK, OK]
        _bitwise(_row(r, 0), _row(r, 1))
        _check_parity(r, 1, t, "negated quaternions", lin)


def test_non_finite_windows_fail_alone(ctx):
    """a NaN in a pose quaternion or in a record's delta_q: NUMERIC, a zero step, NaN costs, nothing written; the neighbours are what they
    are alone"""
    from cerberus_amd import api
    good = shape_window("L70")
    bad_pose = good.twin()
    bad_pose.pose[4, 4] = np.nan
    bad_rec = shape_window("L9").twin()
    bad_rec.preint = shape_window("L9").preint.copy()
    bad_rec.preint[7, 5] = np.nan   # delta_q.y of interval 7
    alone = _row(api.Batch(ctx, [good.twin()]).gyro_bias_align("corrected"), 0)
    ws = [bad_pose, good.twin(), bad_rec, good.twin()]
    b = api.Batch(ctx, ws)
    before = _state(ws)
    for write in (False, True):
        r = b.gyro_bias_align("corrected", write=write)
        assert list(r.status) == [NUMERIC, OK, NUMERIC, OK] and list(r.n_intervals) == [10] * 4
        for i in (0, 2):
            assert not r.delta_bg[i].any() and np.isnan(r.initial_cost[i]) and np.isnan(r.model_cost[i])
        for i in (1, 3):
            _bitwise(_row(r, i), alone)
    b.download()
    after = _state(ws)
    for i in (0, 2):
        for x, y in zip(after[6 * i:6 * i + 6], before[6 * i:6 * i + 6]):
            assert x.tobytes() == y.tobytes()
    assert after[7].tobytes() != before[7].tobytes()   # (the good windows were written)


def _integration_bound(p, lin, rng):
    """ten times the change of the definition's step when its record inputs move by what tests/test_golden.py allows between two
    integrations of the same samples (_check_records: state entries rtol 1e-11 + atol 1e-13, Jacobian entries rtol 1e-9 + atol 1e-11)"""
    ref = gyro_ref.align_parts(p, lin)
    worst = 0.0
    for _ in range(8):
        s1, s2 = rng.choice([-1.0, 1.0], p.dq.shape), rng.choice([-1.0, 1.0], p.J.shape)
        m = p._replace(dq=p.dq + s1 * (1e-11 * np.abs(p.dq) + 1e-13), J=p.J + s2 * (1e-9 * np.abs(p.J) + 1e-11))
        worst = max(worst, gyro_ref.step_error(gyro_ref.align_parts(m, lin).delta_bg, ref.delta_bg))
    return 10.0 * worst


def test_samples_in_force(ctx, cfg, ocfg):
    from cerberus_amd import api
    rng = np.random.default_rng(5)
    base = []
    for s in (31, 32):
        w = _window(cfg, ocfg, seed=s, L=40)
        w.speed_bias[:, 3:6] += 2e-2 * rng.normal(size=(11, 3))
        w.speed_bias[:, 6:9] += 2e-3 * rng.normal(size=(11, 3))
        w.leg_bias += 2e-3 * rng.normal(size=(11, 4))
        base.append(w)
    # before any solve: the records sit at their own linearisation point, the state's biases elsewhere
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    b.set_samples()
    recs0 = [b.fetch(13, i).tobytes() for i in range(2)]
    bytes0 = b.device_bytes()
    rs = [b.gyro_bias_align(lin) for lin in LINS]
    assert b.device_bytes() == bytes0
    assert [b.fetch(13, i).tobytes() for i in range(2)] == recs0
    assert rs[0].delta_bg.tobytes() == rs[1].delta_bg.tobytes() and list(rs[0].status) == [OK, OK]
    for i, w in enumerate(ws):
        lin10 = np.concatenate([w.speed_bias[:10, 3:9], w.leg_bias[:10]], axis=1)
        rec = ctx.preintegrate(w.samples[:int(w.sample_offsets[-1])], w.sample_offsets, lin10)
        np.testing.assert_array_equal(rec[:, 26:29], w.speed_bias[:10, 6:9])
        for k, lin in enumerate(LINS):
            tol = _integration_bound(gyro_ref.parts(w, rec), lin, rng)
            print("MEASURED samples window %d %s: bound %.1e (ten times the change under the integrations' allowed difference)" % (i, lin, tol))
            _check_parity(rs[k], i, w, "samples window %d" % i, lin, rec=rec, tol=tol)
        # on the batch's own records, integrated at another point, the record form gives another step
        assert gyro_ref.step_error(gyro_ref.align(w, "record").delta_bg, rs[0].delta_bg[i]) > 100 * gyro_ref.TOL
    # after a solve (the records may sit at a rejected candidate): the call changes neither them nor the solve that follows
    opts = api.default_solve_opts(True, 4)
    st_a, su_a, re_a, rc_a = _sequence(ctx, base, opts, False, samples=True)[:4]
    st_b, su_b, re_b, rc_b, out, wb = _sequence(ctx, base, opts, True, samples=True)
    for x, y in zip(st_a, st_b):
        assert x.tobytes() == y.tobytes()
    assert su_a == su_b and re_a == re_b and rc_a == rc_b
    assert out[0].delta_bg.tobytes() == out[1].delta_bg.tobytes() and list(out[0].status) == [OK, OK]


def test_host_window_form_matches_batch(ctx):
    from cerberus_amd import api
    ws = [shape_window("L70").twin(), _singular(shape_window("L9")), shape_window("F6").twin()]
    for lin in LINS:
        r = api.Batch(ctx, [w.twin() for w in ws]).gyro_bias_align(lin)
        tw = [w.twin() for w in ws]
        h = ctx.window_gyro_bias_align(tw, lin)
        for i in range(3):
            _bitwise(_row(h, i), _row(r, i))
            for x, y in zip(tw[i].state_arrays(), ws[i].state_arrays()):
                assert x.tobytes() == y.tobytes()   # write = 0: the windows are left alone
        tw = [w.twin() for w in ws]
        h = ctx.window_gyro_bias_align(tw, lin, write=True)
        for i in range(3):
            _bitwise(_row(h, i), _row(r, i))
            want = ws[i].speed_bias.copy()
            if h.status[i] == OK:
                want[:ws[i].F, 6:9] = want[:ws[i].F, 6:9] + h.delta_bg[i]
            assert tw[i].speed_bias.tobytes() == want.tobytes()
            for j, (x, y) in enumerate(zip(tw[i].state_arrays(), ws[i].state_arrays())):
                assert j == 1 or x.tobytes() == y.tobytes()
    assert list(h.status) == [OK, SINGULAR, OK]
    # USE_LEG = 0 through the host form (a batch of its own: one IMU factor kind per batch)
    imu = kind_window("L9", 0)
    h = ctx.window_gyro_bias_align([imu.twin()])
    _check_parity(h, 0, imu, "host form use_leg 0", "record")


def test_device_memory_is_returned(ctx, cfg, ocfg):
    from cerberus_amd import api
    b = api.Batch(ctx, [_window(cfg, ocfg, seed=s, L=50) for s in (13, 14)])
    bytes0 = b.device_bytes()
    first = b.gyro_bias_align()
    assert b.device_bytes() == bytes0
    for _ in range(20):
        r = b.gyro_bias_align()
        assert b.device_bytes() == bytes0
    for i in range(2):
        _bitwise(_row(r, i), _row(first, i))


def test_bad_arguments(ctx):
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    w = shape_window("L9").twin()
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_gyro_bias_align
    d, rec = np.zeros(3), (T.WindowGyroRecord * 1)()
    pd = d.ctypes.data_as(T.c_double_p)

    def opts(**kw):
        o = T.GyroOpts()
        api.lib().vilo_default_gyro_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    assert f(None, b.handle, opts(), pd, rec) == -2
    assert f(ctx.h, None, opts(), pd, rec) == -2
    assert f(ctx.h, b.handle, opts(), None, rec) == -2          # NULL delta_bg with windows present
    for bad in (2, -1):
        assert f(ctx.h, b.handle, opts(linearization=bad), pd, rec) == -2
    for bad in (2, -1):
        assert f(ctx.h, b.handle, opts(write=bad), pd, rec) == -2
    g = api.lib().vilo_window_gyro_bias_align
    ds, ss = w.desc(T)
    assert g(ctx.h, 0, C.byref(ds), C.byref(ss), opts(), pd, rec) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(linearization=7), pd, rec) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(), None, rec) == -2
    assert not d.any() and rec[0].status == 0 and rec[0].n_intervals == 0
    b.download()
    assert w.speed_bias.tobytes() == shape_window("L9").speed_bias.tobytes()   # (write = 2 wrote nothing)
    # the batch is still usable; NULL options are the defaults, the records may be left out
    assert f(ctx.h, b.handle, None, pd, None) == 0
    r = b.gyro_bias_align()
    assert d.tobytes() == r.delta_bg[0].tobytes() and r.status[0] == OK
    assert api.lib().vilo_last_gyro_align_ms(ctx.h) > 0.0
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(), pd, rec) == 0 and rec[0].status == OK and rec[0].n_intervals == 10
    assert d.tobytes() == r.delta_bg[0].tobytes()
