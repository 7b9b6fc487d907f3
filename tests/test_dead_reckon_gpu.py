"""GPU (-m gpu): vilo_batch_dead_reckon / vilo_window_dead_reckon against the numpy definition (tests/deadreckon_ref.py) at the state the
device returns: windows of 2, 3, 6 and 11 frames with ranges of 0, 1, 2 and 30 samples side by side, leg and IMU-only batches, the
default configuration and tests/alt_config.py's, the initial state and the state after a solve, the last frame and an explicit one;
independence of batch size and position; freedom from side effects; the write-back and what follows it (solve, graph replay, reset);
the statuses; the host form; the hand-over to predict_next_frame; the host window manager; bad arguments. Tolerance: ten times the FP64
floor tests/test_dead_reckon.py measures (deadreckon_ref.TOL); n_steps and statuses exactly."""
import ctypes as C

import numpy as np
import pytest

import alt_config
import deadreckon_ref as D
from test_covariance_gpu import _window
from test_dead_reckon import RANGES, frames_window, take
from test_gyro_align import kind_window

pytestmark = pytest.mark.gpu

OK, NO_FRAME, NUMERIC = D.OK, D.NO_FRAME, D.NUMERIC


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def actx(cfg):
    from cerberus_amd import api
    c = api.Context(alt_config.alt_config(cfg), 0)
    yield c
    c.close()


def _pack(ranges):
    """(samples [sum n, 35], offsets [W + 1]) of one range [n, 35] per window"""
    off = np.zeros(len(ranges) + 1, np.int32)
    off[1:] = np.cumsum([len(r) for r in ranges])
    return np.ascontiguousarray(np.concatenate([np.reshape(r, (-1, 35)) for r in ranges])), off


def _part(r, i):
    """window i's outputs, every array of them"""
    out = [np.ascontiguousarray(r.state[i]), np.asarray(r.n_steps[i]), np.asarray(r.status[i])]
    if r.trajectory is not None:
        out.append(np.ascontiguousarray(r.trajectory[r.step_offsets[i]:r.step_offsets[i + 1]]))
    return out


def _bitwise(x, y):
    for a, b in zip(x, y):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert a.tobytes() == b.tobytes()


def _state(ws):
    return [a.copy() for w in ws for a in w.state_arrays()]


def _check_parity(r, i, w, rng_i, g, f, tag, write=False, want=OK):
    """window i of the report against the definition at w's state arrays; returns the largest error of its rows"""
    ref = D.window_dead_reckon(w, rng_i, g, f, write)
    assert ref.status == want and r.status[i] == want, (tag, ref.status, r.status[i])
    assert r.n_steps[i] == ref.n_steps == max(0, len(rng_i) - 1) == r.step_offsets[i + 1] - r.step_offsets[i], tag
    e = D.state_error(r.state[i], ref.state) if want == OK else 0.0
    et = 0.0
    if r.trajectory is not None:
        t = r.trajectory[r.step_offsets[i]:r.step_offsets[i + 1]]
        if want == OK:
            et = D.rows_error(t, ref.trajectory)
            if ref.n_steps:
                assert t[-1].tobytes() == r.state[i].tobytes(), tag   # the last row is state_out, bit for bit
        else:
            assert not t.any(), tag
    if want != OK:
        assert not r.state[i].any(), tag
    print("MEASURED %s: state %.1e, trajectory %.1e (tolerance %.0e), %d steps" % (tag, e, et, D.TOL, ref.n_steps))
    assert max(e, et) <= D.TOL, (tag, e, et)
    return max(e, et)


GROUPS = {
    #          windows                                                            explicit frame, solved too
    "leg": (lambda: [kind_window("L9", 1), kind_window("F6", 1)], 4, True),
    "imu_only": (lambda: [kind_window("L9", 0)], 9, True),
    "short": (lambda: [frames_window(3), frames_window(2)], 0, False),   # (frame 0: the only frame before a two-frame window's last)
}


@pytest.mark.parametrize("which", ["default", "alt"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_parity_with_numpy(ctx, actx, cfg, group, which):
    """every window of the group with a range of 0, 1, 2 and 30 samples in ONE batch; from the last frame and from an explicit one; at the
    initial state and after a 4-iteration solve; with and without the trajectory (the same state bits)"""
    from cerberus_amd import api
    c = actx if which == "alt" else ctx
    g = alt_config.alt_config(cfg).g_norm if which == "alt" else cfg.g_norm
    make, explicit, solve = GROUPS[group]
    ws = [w.twin() for w in make() for _ in RANGES]
    ranges = [take(w, RANGES[i % len(RANGES)], 3 * i) for i, w in enumerate(ws)]
    samples, offsets = _pack(ranges)
    b = api.Batch(c, ws)
    worst = 0.0
    for state in ("initial", "solved") if solve and which == "default" else ("initial",):
        if state == "solved":
            b.solve(api.default_solve_opts(True, 4))
            b.download()
        for f in (-1, explicit):
            r = b.dead_reckon(samples, offsets, f, trajectory=True)
            assert list(r.step_offsets) == list(np.concatenate([[0], np.cumsum([max(0, len(x) - 1) for x in ranges])]))
            assert r.trajectory.shape == (r.step_offsets[-1], 10)
            for i, w in enumerate(ws):
                worst = max(worst, _check_parity(r, i, w, ranges[i], g, f, "%s %s %s window %d (%d frames) from_frame %d" % (group, which, state, i, w.F, f)))
            r0 = b.dead_reckon(samples, offsets, f)
            assert r0.trajectory is None and r0.state.tobytes() == r.state.tobytes() and r0.status.tobytes() == r.status.tobytes()
    print("MEASURED %s %s: largest error %.1e (floor %.0e, tolerance %.0e)" % (group, which, worst, D.FLOOR, D.TOL))


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg):
    """alone, at position 3 of 8 and at positions 0 / 150 / 299 of 300 windows of other shapes and range lengths (five workgroups, the last
    one partial): bit for bit the same, for a long range and for a one-step range of a short window"""
    from cerberus_amd import api
    subjects = [(kind_window("L9", 1), take(kind_window("L9", 1), 30, 2)), (frames_window(3), take(frames_window(3), 2, 40))]
    others = [_window(cfg, ocfg, seed=78, L=30), kind_window("F6", 1), frames_window(2)]
    for f in (-1, 1):
        for w, s in subjects:
            def run(ws, rs):
                smp, off = _pack(rs)
                return api.Batch(ctx, ws).dead_reckon(smp, off, f, trajectory=True)
            alone = _part(run([w.twin()], [s]), 0)
            assert alone[2] == OK and alone[1] == len(s) - 1

            def crowd(n, at):
                ws = [others[i % 3].twin() for i in range(n)]
                rs = [take(ws[i], RANGES[(i + 1) % 4], i % 50) for i in range(n)]
                for p in at:
                    ws[p], rs[p] = w.twin(), s
                return run(ws, rs)
            _bitwise(_part(crowd(8, [3]), 3), alone)
            r = crowd(300, [0, 150, 299])
            for p in (0, 150, 299):
                _bitwise(_part(r, p), alone)


def _sequence(ctx, base, opts, report):
    from cerberus_amd import api
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    b.solve(opts)
    summ0 = b.download()
    before = _state(ws)
    if report:
        smp, off = _pack([take(w, 30, 4 * i) for i, w in enumerate(ws)])
        bytes0 = b.device_bytes()
        first = b.dead_reckon(smp, off, trajectory=True)
        assert b.device_bytes() == bytes0   # nothing is kept with the batch: not even at the first call
        for f in (-1, 3):
            r = b.dead_reckon(smp, off, f, trajectory=(f == -1))
            assert b.device_bytes() == bytes0 and list(r.status) == [OK] * len(ws)
        _bitwise(_part(r, 0)[:3], _part(b.dead_reckon(smp, off, 3), 0)[:3])
        _bitwise(_part(first, 1), _part(b.dead_reckon(smp, off, trajectory=True), 1))
        summ1 = b.download()
        for x, y in zip(before, _state(ws)):
            assert x.tobytes() == y.tobytes()
        assert [bytes(s) for s in summ0] == [bytes(s) for s in summ1]
    b.solve(opts)
    replay = b.path()["replay"]
    summ = b.download()
    return _state(ws), [bytes(s) for s in summ], replay


def test_no_side_effects(ctx, cfg, ocfg):
    """solve, dead-reckon (write = 0), download: states and summaries bit for bit unchanged and device_bytes() where it was; the solve that
    follows (a replay of the captured graph) is bit for bit what it is without the calls"""
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s, L=60) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)
    st_a, su_a, rp_a = _sequence(ctx, base, opts, False)
    st_b, su_b, rp_b = _sequence(ctx, base, opts, True)
    for x, y in zip(st_a, st_b):
        assert x.tobytes() == y.tobytes()
    assert su_a == su_b and rp_a == rp_b and rp_b   # the second solve of a batch replays the graph the first one captured


@pytest.mark.parametrize("replay", [False, True])
def test_write_back(ctx, replay):
    from cerberus_amd import api
    opts = api.default_solve_opts(True, 4)
    base = [kind_window("L70", 1).twin(), kind_window("L9", 1).twin(), kind_window("F6", 1).twin()]
    f = 4
    ws = [w.twin() for w in base]
    ranges = [take(w, n, 7 * i) for i, (w, n) in enumerate(zip(ws, (30, 2, 30)))]
    smp, off = _pack(ranges)
    b = api.Batch(ctx, ws)
    if replay:
        b.solve(opts)   # solve once before the write: the solve after it replays the captured graph
        b.reset()
    b.download()
    before = _state(ws)
    dry = b.dead_reckon(smp, off, f, trajectory=True)
    r = b.dead_reckon(smp, off, f, write=True, trajectory=True)
    assert list(r.status) == [OK] * 3
    for i in range(3):
        _bitwise(_part(r, i), _part(dry, i))
    b.download()
    after = _state(ws)
    for i, w in enumerate(ws):
        for j in range(6):
            x, y = after[6 * i + j], before[6 * i + j].copy()
            if j == 0:      # pose: row f + 1 is [P, q] of state_out, every other row as it was
                y[f + 1] = r.state[i, 0:7]
            if j == 1:      # speed_bias: the velocity of row f + 1; its biases and every other row as they were
                y[f + 1, 0:3] = r.state[i, 7:10]
            if j < 2:
                assert x.tobytes() != before[6 * i + j].tobytes()
            assert x.tobytes() == y.tobytes(), (i, j)
    # the solve after it starts from the new state: bit for bit the solve of a batch created with those states
    fresh = [w.twin() for w in ws]
    b.solve(opts)
    assert b.path()["replay"] == replay
    b.download()
    fb = api.Batch(ctx, fresh)
    fb.solve(opts)
    fb.download()
    for w, fw in zip(ws, fresh):
        for x, y in zip(w.state_arrays(), fw.state_arrays()):
            assert x.tobytes() == y.tobytes()
    # the uploaded initial state is still what reset restores
    b.reset()
    b.download()
    for w, o in zip(ws, base):
        for x, y in zip(w.state_arrays(), o.state_arrays()):
            assert x.tobytes() == y.tobytes()


def test_statuses(ctx, cfg):
    """a 2-frame window between 11-frame ones: NO_FRAME with from_frame 5, and with from_frame 1 plus write (it has no frame 2); a NaN in
    one window's start velocity, or in one of its samples: NUMERIC there alone. The failing window reports zeros and is not written; its
    neighbours are bit for bit what they are alone."""
    from cerberus_amd import api
    g = cfg.g_norm
    full, two = kind_window("L9", 1), frames_window(2)
    ranges = [take(full, 30, 0), take(two, 30, 9), take(full, 2, 20)]
    smp, off = _pack(ranges)

    def alone(w, s, f, write=False):
        a, o = _pack([s])
        return _part(api.Batch(ctx, [w.twin()]).dead_reckon(a, o, f, write=write, trajectory=True), 0)
    for f, write, want in ((5, False, NO_FRAME), (1, True, NO_FRAME), (1, False, OK)):
        ws = [full.twin(), two.twin(), full.twin()]
        b = api.Batch(ctx, ws)
        r = b.dead_reckon(smp, off, f, write=write, trajectory=True)
        assert list(r.status) == [OK, want, OK] and list(r.n_steps) == [29, 29, 1]
        for i, w in enumerate(ws):
            _check_parity(r, i, w, ranges[i], g, f, "2 frames between 11, from_frame %d write %d, window %d" % (f, write, i), write, r.status[i])
        for i in (0, 2):
            _bitwise(_part(r, i), alone(full, ranges[i], f, write))
        b.download()
        for x, y in zip(ws[1].state_arrays(), two.state_arrays()):
            assert x.tobytes() == y.tobytes()
        assert (ws[0].pose.tobytes() != full.pose.tobytes()) == write   # (the neighbours were written)
    # not finite: the start velocity of the middle window; one sample value of the middle window (a gyro component of its 8th sample)
    for kind in ("velocity", "sample"):
        ws = [full.twin(), full.twin(), full.twin()]
        rs = [take(full, 30, 0), take(full, 30, 3).copy(), take(full, 2, 20)]
        if kind == "velocity":
            ws[1].speed_bias[5, 1] = np.nan
        else:
            rs[1][7, 5] = np.nan
        a, o = _pack(rs)
        for write in (False, True):
            b = api.Batch(ctx, ws)
            r = b.dead_reckon(a, o, 5, write=write, trajectory=True)
            assert list(r.status) == [OK, NUMERIC, OK], kind
            _check_parity(r, 1, ws[1], rs[1], g, 5, "NaN in a %s" % kind, write, NUMERIC)
            for i in (0, 2):
                _bitwise(_part(r, i), alone(full, rs[i], 5, write))
            got = [w.twin() for w in ws]
            bb = api.Batch(ctx, got)
            bb.dead_reckon(a, o, 5, write=write)
            bb.download()
            for x, y in zip(got[1].state_arrays(), ws[1].state_arrays()):
                assert x.tobytes() == y.tobytes()   # nothing of the failing window is written
            assert (got[0].pose.tobytes() != ws[0].pose.tobytes()) == write
    # the same NaN in another frame's velocity, or in a sample no range reads, fails nothing
    ws = [full.twin()]
    ws[0].speed_bias[6, 1] = np.nan
    a, o = _pack([take(full, 30, 0)])
    assert api.Batch(ctx, ws).dead_reckon(a, o, 5).status[0] == OK
    # offsets that decrease, or do not start at 0, raise
    b = api.Batch(ctx, [full.twin(), full.twin()])
    for bad in ([0, 5, 3], [1, 5, 9], [0, 5]):
        with pytest.raises(ValueError):
            b.dead_reckon(take(full, 30, 0), bad)


def test_host_window_form_matches_batch(ctx):
    from cerberus_amd import api
    ws = [kind_window("L70", 1).twin(), frames_window(2).twin(), kind_window("F6", 1).twin()]
    smp, off = _pack([take(w, n, 5 * i) for i, (w, n) in enumerate(zip(ws, (30, 30, 1)))])
    for f, write in ((-1, False), (1, False), (1, True)):
        r = api.Batch(ctx, [w.twin() for w in ws]).dead_reckon(smp, off, f, trajectory=True)
        tw = [w.twin() for w in ws]
        h = ctx.window_dead_reckon(tw, smp, off, f, write=write, trajectory=True)
        assert list(h.status) == [OK, NO_FRAME if write else OK, OK]
        for i in range(3):
            if h.status[i] == r.status[i]:
                _bitwise(_part(h, i), _part(r, i))
            want_pose, want_sb = ws[i].pose.copy(), ws[i].speed_bias.copy()
            if write and h.status[i] == OK:
                want_pose[f + 1], want_sb[f + 1, 0:3] = h.state[i, 0:7], h.state[i, 7:10]
            assert tw[i].pose.tobytes() == want_pose.tobytes() and tw[i].speed_bias.tobytes() == want_sb.tobytes()
            for x, y in zip(tw[i].state_arrays()[2:], ws[i].state_arrays()[2:]):
                assert x.tobytes() == y.tobytes()
    # USE_LEG = 0 through the host form (a batch of its own: one IMU factor kind per batch)
    imu = kind_window("L9", 0)
    a, o = _pack([take(imu, 30, 1)])
    _bitwise(_part(ctx.window_dead_reckon([imu.twin()], a, o), 0), _part(api.Batch(ctx, [imu.twin()]).dead_reckon(a, o), 0))


def test_hand_over_to_predict_next_frame(ctx):
    """the dead-reckoned pose is what predict_next_frame's given mode takes: OK, and next_pose is the input with its quaternion normalised"""
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    ws = [kind_window("L70", 1).twin(), kind_window("L9", 1).twin(), kind_window("F6", 1).twin()]
    smp, off = _pack([take(w, 30, 6 * i) for i, w in enumerate(ws)])
    b = api.Batch(ctx, ws)
    b.solve(api.default_solve_opts(True, 4))
    r = b.dead_reckon(smp, off)
    assert list(r.status) == [OK] * 3
    p = b.predict_next_frame("given", r.state[:, 0:7])
    assert list(p.status) == [T.PREDICT_OK] * 3 and p.n_predicted.min() > 0
    for i in range(3):
        q = r.state[i, 3:7]
        assert p.next_pose[i, 0:3].tobytes() == r.state[i, 0:3].tobytes()
        # (a square root and a division away from the input: two roundings of values below 1)
        assert np.abs(p.next_pose[i, 3:7] - D.quat_normalized(q)).max() <= 2 * np.finfo(float).eps


def test_host_window_manager(ctx, cfg):
    """sequence.SlidingWindow (SlidingWindow::processIMULeg, the one-robot host form) fed the same samples from the same start ends at a
    newest-frame P, R, V within the tolerance of the call's (the host compiler may contract and adds in another order: not bitwise)"""
    from cerberus_amd import api, sequence
    w = kind_window("L9", 1).twin()
    f = w.F - 1
    w.speed_bias[f, 3:9] = 0.0   # the manager's biases are zero until its first solve
    s = take(w, 30, 5)
    sw = sequence.SlidingWindow(ctx, cfg)
    sw.init_first_pose(w.pose[f, 0:3], D.quat_R(D.quat_normalized(w.pose[f, 3:7])).ravel(), w.speed_bias[f, 0:3])
    sw.process_samples(s[:1])   # frame 0: nothing is propagated, the sample becomes (acc_0, gyr_0)
    first = [l for l in range(w.L) if w.lm_start_frame[l] == 0]
    rows = [w.lm_obs_offset[l] for l in first]
    sw.process_image(0.0, np.array(first, np.int32), w.obs[rows], w.obs_is_stereo[rows])   # the newest frame becomes a copy of frame 0
    assert sw.state()["frame_count"] == 1
    sw.process_samples(s[1:])
    st = sw.state()
    a, o = _pack([s])
    r = api.Batch(ctx, [w]).dead_reckon(a, o)
    assert r.status[0] == OK and r.n_steps[0] == 29
    # the manager's R goes through the same Quaterniond(R) as the call's before the metric takes both back to matrices (R itself is not a
    # rotation to fourth order in |un_gyr dt|, so it is not the matrix of its own quaternion)
    eP, eV, eR = D.state_errors(np.concatenate([st["Ps"][1], D.quat_from_R(st["Rs"][1]), st["Vs"][1]]), r.state[0])
    print("MEASURED host window manager: P %.1e V %.1e R %.1e (tolerance %.0e)" % (eP, eV, eR, D.TOL))
    assert max(eP, eV, eR) <= D.TOL


def test_bad_arguments(ctx, cfg):
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    w = kind_window("L9", 1).twin()
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_dead_reckon
    smp, off = _pack([take(w, 30, 0)])
    st, tr, rec = np.zeros((1, 10)), np.zeros((29, 10)), (T.WindowDeadReckonRecord * 1)()
    ps, po, pst, ptr = C.cast(smp.ctypes.data, C.POINTER(T.Sample)), T.iptr(off), st.ctypes.data_as(T.c_double_p), tr.ctypes.data_as(T.c_double_p)

    def opts(**kw):
        o = T.DeadReckonOpts()
        api.lib().vilo_default_dead_reckon_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    assert f(None, b.handle, opts(), ps, po, pst, ptr, rec) == -2
    assert f(ctx.h, None, opts(), ps, po, pst, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(), ps, None, pst, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(), ps, po, None, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(), None, po, pst, ptr, rec) == -2          # NULL samples with samples to read
    for bad in (-2, T.MAX_FRAMES):
        assert f(ctx.h, b.handle, opts(from_frame=bad), ps, po, pst, ptr, rec) == -2
    for bad in (2, -1):
        assert f(ctx.h, b.handle, opts(from_frame=3, write=bad), ps, po, pst, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(write=1), ps, po, pst, ptr, rec) == -2   # write without a frame: no target
    assert b"from_frame" in api.lib().vilo_last_error(ctx.h)
    for bad in ([1, 30], [0, -1], [30, 0]):
        bo = np.array(bad, np.int32)
        assert f(ctx.h, b.handle, opts(), ps, T.iptr(bo), pst, ptr, rec) == -2
    g = api.lib().vilo_window_dead_reckon
    ds, ss = w.desc(T)
    assert g(ctx.h, 0, C.byref(ds), C.byref(ss), opts(), ps, po, pst, ptr, rec) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(write=1), ps, po, pst, ptr, rec) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(from_frame=11), ps, po, pst, ptr, rec) == -2
    assert not st.any() and not tr.any() and rec[0].n_steps == 0 and rec[0].status == 0
    b.download()
    assert w.pose.tobytes() == kind_window("L9", 1).pose.tobytes() and w.speed_bias.tobytes() == kind_window("L9", 1).speed_bias.tobytes()
    # the batch is still usable; NULL options are the defaults, the trajectory and the records may be left out; no samples at all
    assert f(ctx.h, b.handle, None, ps, po, pst, None, None) == 0
    r = b.dead_reckon(smp, off, trajectory=True)
    assert st.tobytes() == r.state.tobytes() and r.status[0] == OK and not tr.any()
    assert api.lib().vilo_last_dead_reckon_ms(ctx.h) > 0.0
    assert f(ctx.h, b.handle, opts(), ps, po, pst, ptr, rec) == 0 and (rec[0].status, rec[0].n_steps) == (OK, 29)
    assert tr.tobytes() == r.trajectory.tobytes()
    zero = np.zeros(2, np.int32)
    assert f(ctx.h, b.handle, opts(), None, T.iptr(zero), pst, ptr, rec) == 0 and (rec[0].status, rec[0].n_steps) == (OK, 0)
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), None, ps, po, pst, ptr, rec) == 0 and st.tobytes() == r.state.tobytes()
    _check_parity(r, 0, w, take(w, 30, 0), cfg.g_norm, -1, "after bad arguments")
