"""GPU (-m gpu): vilo_batch_dead_reckon_covariance / vilo_window_dead_reckon_covariance against the numpy definition (tests/drcov_ref.py)
at the state the device returns: windows of 2, 3, 6 and 11 frames with ranges of 0, 1, 2 and 30 samples of unequal dt side by side, leg
and IMU-only batches, the default configuration and tests/alt_config.py's, cov_in NULL, given, and cut from Batch.covariance() after a
4-iteration solve, the last frame and an explicit one; the state bit for bit Batch.dead_reckon's; symmetry, the smallest eigenvalue and
the last trajectory row; independence of batch size and position; freedom from side effects; the statuses; the host form; bad arguments.
Tolerance: ten times the FP64 floor tests/test_dr_covariance.py measures (drcov_ref.TOL); n_steps and statuses exactly."""
import ctypes as C

import numpy as np
import pytest

import alt_config
import drcov_ref as DC
from test_covariance_gpu import _window
from test_dead_reckon import RANGES, frames_window
from test_dr_covariance import given_cov, take
from test_gyro_align import kind_window

pytestmark = pytest.mark.gpu

OK, NO_FRAME, NUMERIC = DC.OK, DC.NO_FRAME, DC.NUMERIC


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
    out = [np.ascontiguousarray(r.state[i]), np.ascontiguousarray(r.cov[i]), np.asarray(r.n_steps[i]), np.asarray(r.status[i])]
    if r.pose_cov_trajectory is not None:
        out.append(np.ascontiguousarray(r.pose_cov_trajectory[r.step_offsets[i]:r.step_offsets[i + 1]]))
    return out


def _bitwise(x, y):
    assert len(x) == len(y)
    for a, b in zip(x, y):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert a.tobytes() == b.tobytes()


def _state(ws):
    return [a.copy() for w in ws for a in w.state_arrays()]


def _check_parity(r, i, w, rng_i, g, noise, f, cov_in, tag, want=OK):
    """window i of the report against the definition at w's state arrays; returns the largest error of its covariances"""
    ref = DC.window_dr_cov(w, rng_i, g, noise, f, cov_in)
    assert ref.status == want and r.status[i] == want, (tag, ref.status, r.status[i])
    assert r.n_steps[i] == ref.n_steps == max(0, len(rng_i) - 1) == r.step_offsets[i + 1] - r.step_offsets[i], tag
    cov = r.cov[i]
    assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes(), tag   # bitwise symmetric
    e = et = 0.0
    t = None if r.pose_cov_trajectory is None else r.pose_cov_trajectory[r.step_offsets[i]:r.step_offsets[i + 1]]
    if want == OK:
        e = DC.cov_error(cov, ref.cov)
        assert np.linalg.eigvalsh(cov).min() >= -DC.FLOOR * np.trace(cov), tag
        if ref.n_steps == 0:
            assert cov.tobytes() == ref.cov.tobytes(), tag   # no step: the mirrored input, bit for bit
        if t is not None:
            et = DC.rows_error(t, ref.pose_cov_trajectory)
            assert t.tobytes() == np.ascontiguousarray(np.swapaxes(t, 1, 2)).tobytes(), tag
            if ref.n_steps:
                assert t[-1].tobytes() == np.ascontiguousarray(cov[:6, :6]).tobytes(), tag   # the last row is cov_out's pose block
    else:
        assert not cov.any() and not r.state[i].any() and (t is None or not t.any()), tag
    print("MEASURED %s: cov %.1e, trajectory %.1e (tolerance %.0e), %d steps" % (tag, e, et, DC.TOL, ref.n_steps))
    assert max(e, et) <= DC.TOL, (tag, e, et)
    return max(e, et)


GROUPS = {
    #          windows                                                            explicit frame, which cov_in
    "leg": (lambda: [kind_window("L9", 1), kind_window("F6", 1)], 4, ("null", "solved")),
    "imu_only": (lambda: [kind_window("L9", 0)], 9, ("null", "solved")),
    "short": (lambda: [frames_window(3), frames_window(2)], 0, ("null", "given")),   # (frame 0: the only frame before a two-frame window's last)
}


@pytest.mark.parametrize("which", ["default", "alt"])
@pytest.mark.parametrize("group", sorted(GROUPS))
def test_parity_with_numpy(ctx, actx, cfg, group, which):
    """every window of the group with a range of 0, 1, 2 and 30 samples in ONE batch; from the last frame and from an explicit one; at the
    initial state with cov_in NULL (the short windows also with a given one) and after a 4-iteration solve with cov_in cut from the
    batch's own covariance; with and without the trajectory (the same bits); the state bit for bit dead_reckon's"""
    from cerberus_amd import api
    c, acfg = (actx, alt_config.alt_config(cfg)) if which == "alt" else (ctx, cfg)
    g, noise = acfg.g_norm, DC.noise_of(acfg)
    make, explicit, kinds = GROUPS[group]
    if which == "alt":
        kinds = ("null", "given")   # (the windows' records are integrated at the default configuration: no solve at the other one)
    ws = [w.twin() for w in make() for _ in RANGES]
    ranges = [take(w, RANGES[i % len(RANGES)], 3 * i) for i, w in enumerate(ws)]
    samples, offsets = _pack(ranges)
    nf = np.array([w.F for w in ws])
    b = api.Batch(c, ws)
    worst = 0.0
    for kind in kinds:
        if kind == "solved":
            b.solve(api.default_solve_opts(True, 4))
            b.download()
            frames, _, cst = b.covariance(gauge="frame0")
            assert not cst.any(), cst
        for f in (-1, explicit):
            cov_in = None
            if kind == "given":
                cov_in = np.array([given_cov(i) for i in range(len(ws))])
            if kind == "solved":
                cov_in = api.dr_cov_in(frames, nf, f)
            r = b.dead_reckon_covariance(samples, offsets, cov_in, f, pose_trajectory=True)
            assert list(r.step_offsets) == list(np.concatenate([[0], np.cumsum([max(0, len(x) - 1) for x in ranges])]))
            assert r.pose_cov_trajectory.shape == (r.step_offsets[-1], 6, 6) and r.cov.shape == (len(ws), 15, 15)
            for i, w in enumerate(ws):
                worst = max(worst, _check_parity(r, i, w, ranges[i], g, noise, f, None if cov_in is None else cov_in[i],
                                                 "%s %s %s window %d (%d frames) from_frame %d" % (group, which, kind, i, w.F, f)))
            r0 = b.dead_reckon_covariance(samples, offsets, cov_in, f)
            assert r0.pose_cov_trajectory is None
            assert r0.state.tobytes() == r.state.tobytes() and r0.cov.tobytes() == r.cov.tobytes() and r0.status.tobytes() == r.status.tobytes()
            d = b.dead_reckon(samples, offsets, f)
            assert d.state.tobytes() == r.state.tobytes() and d.status.tobytes() == r.status.tobytes() and d.n_steps.tobytes() == r.n_steps.tobytes()
    print("MEASURED %s %s: largest error %.1e (floor %.0e, tolerance %.0e)" % (group, which, worst, DC.FLOOR, DC.TOL))


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg):
    """alone, at position 3 of 8 and at positions 0 / 150 / 299 of 300 windows of other frame counts and range lengths (75 waves of four
    windows: positions 150 and 299 sit at lanes 32 .. 47 and 48 .. 63 of theirs, beside ranges of other lengths): bit for bit the same,
    for a long range and for a one-step range of a short window"""
    from cerberus_amd import api
    subjects = [(kind_window("L9", 1), take(kind_window("L9", 1), 30, 2), given_cov(11)), (frames_window(3), take(frames_window(3), 2, 40), None)]
    others = [_window(cfg, ocfg, seed=78, L=30), kind_window("F6", 1), frames_window(2)]
    for f in (-1, 1):
        for w, s, cin in subjects:
            def run(ws, rs, cs):
                smp, off = _pack(rs)
                return api.Batch(ctx, ws).dead_reckon_covariance(smp, off, cs, f, pose_trajectory=True)
            alone = _part(run([w.twin()], [s], None if cin is None else cin[None]), 0)
            assert alone[3] == OK and alone[2] == len(s) - 1

            def crowd(n, at):
                ws = [others[i % 3].twin() for i in range(n)]
                rs = [take(ws[i], RANGES[(i + 1) % 4], i % 50) for i in range(n)]
                cs = np.array([given_cov(100 + i % 7) for i in range(n)])
                for p in at:
                    ws[p], rs[p] = w.twin(), s
                    cs[p] = 0.0 if cin is None else cin
                return run(ws, rs, cs)
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
        cin = np.array([given_cov(i) for i in range(len(ws))])
        bytes0 = b.device_bytes()
        first = b.dead_reckon_covariance(smp, off, cin, pose_trajectory=True)
        assert b.device_bytes() == bytes0   # nothing is kept with the batch: not even at the first call
        for f in (-1, 3):
            r = b.dead_reckon_covariance(smp, off, None if f == 3 else cin, f, pose_trajectory=(f == -1))
            assert b.device_bytes() == bytes0 and list(r.status) == [OK] * len(ws)
        _bitwise(_part(first, 1), _part(b.dead_reckon_covariance(smp, off, cin, pose_trajectory=True), 1))
        summ1 = b.download()
        for x, y in zip(before, _state(ws)):
            assert x.tobytes() == y.tobytes()
        assert [bytes(s) for s in summ0] == [bytes(s) for s in summ1]
    b.solve(opts)
    replay = b.path()["replay"]
    summ = b.download()
    # the landmark mask in force, read last (or-ing nothing into it): after the calls what it is without them
    mask, _ = b.mask_landmarks(mask=np.zeros(sum(w.L for w in ws), np.uint8), combine="or")
    return _state(ws), [bytes(s) for s in summ], replay, np.asarray(mask).tobytes()


def test_no_side_effects(ctx, cfg, ocfg):
    """solve, dead-reckon the covariance, download: states and summaries bit for bit unchanged and device_bytes() where it was; the solve
    that follows (a replay of the captured graph) and the landmark mask are bit for bit what they are without the calls"""
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s, L=60) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)
    st_a, su_a, rp_a, m_a = _sequence(ctx, base, opts, False)
    st_b, su_b, rp_b, m_b = _sequence(ctx, base, opts, True)
    for x, y in zip(st_a, st_b):
        assert x.tobytes() == y.tobytes()
    assert su_a == su_b and rp_a == rp_b and rp_b   # the second solve of a batch replays the graph the first one captured
    assert m_a == m_b


def test_statuses(ctx, cfg):
    """a 2-frame window between 11-frame ones with from_frame 5: NO_FRAME; a NaN in one window's start velocity, in one of its samples, in
    the read triangle of its cov_in: NUMERIC there alone (a NaN below the diagonal is not read). The failing window reports zeros; its
    neighbours are bit for bit what they are alone."""
    from cerberus_amd import api
    g, noise = cfg.g_norm, DC.noise_of(cfg)
    full, two = kind_window("L9", 1), frames_window(2)
    cin = np.array([given_cov(20 + i) for i in range(3)])

    def alone(w, s, f, c):
        a, o = _pack([s])
        return _part(api.Batch(ctx, [w.twin()]).dead_reckon_covariance(a, o, c[None], f, pose_trajectory=True), 0)
    ranges = [take(full, 30, 0), take(two, 30, 9), take(full, 2, 20)]
    smp, off = _pack(ranges)
    for f, want in ((5, NO_FRAME), (1, OK)):
        ws = [full.twin(), two.twin(), full.twin()]
        r = api.Batch(ctx, ws).dead_reckon_covariance(smp, off, cin, f, pose_trajectory=True)
        assert list(r.status) == [OK, want, OK] and list(r.n_steps) == [29, 29, 1]
        for i, w in enumerate(ws):
            _check_parity(r, i, w, ranges[i], g, noise, f, cin[i], "2 frames between 11, from_frame %d, window %d" % (f, i), r.status[i])
        for i in (0, 2):
            _bitwise(_part(r, i), alone(full, ranges[i], f, cin[i]))
    for kind in ("velocity", "sample", "cov_in", "below the diagonal"):
        ws = [full.twin(), full.twin(), full.twin()]
        rs = [take(full, 30, 0), take(full, 30, 3).copy(), take(full, 2, 20)]
        cs = cin.copy()
        if kind == "velocity":
            ws[1].speed_bias[5, 1] = np.nan
        elif kind == "sample":
            rs[1][7, 5] = np.nan
        elif kind == "cov_in":
            cs[1, 3, 11] = np.nan
        else:
            cs[1][np.tril(np.ones((15, 15), bool), -1)] = np.nan
        want = OK if kind == "below the diagonal" else NUMERIC
        a, o = _pack(rs)
        r = api.Batch(ctx, ws).dead_reckon_covariance(a, o, cs, 5, pose_trajectory=True)
        assert list(r.status) == [OK, want, OK], kind
        _check_parity(r, 1, ws[1], rs[1], g, noise, 5, cs[1], "NaN in %s" % kind, want)
        if want == OK:
            _bitwise(_part(r, 1), alone(full, rs[1], 5, cin[1]))
        for i in (0, 2):
            _bitwise(_part(r, i), alone(full, rs[i], 5, cin[i]))
    # the same NaN in another frame's velocity fails nothing; a no-step range with a value that is not finite in its cov_in is NUMERIC too
    ws = [full.twin()]
    ws[0].speed_bias[6, 1] = np.nan
    a, o = _pack([take(full, 30, 0)])
    assert api.Batch(ctx, ws).dead_reckon_covariance(a, o, None, 5).status[0] == OK
    bad = cin[:1].copy()
    bad[0, 0, 0] = np.inf
    a1, o1 = _pack([take(full, 1, 0)])
    r = api.Batch(ctx, [full.twin()]).dead_reckon_covariance(a1, o1, bad)
    assert r.status[0] == NUMERIC and r.n_steps[0] == 0 and not r.cov.any() and not r.state.any()
    # offsets that decrease, or do not start at 0, and a cov_in of another shape raise
    b = api.Batch(ctx, [full.twin(), full.twin()])
    for bad_off in ([0, 5, 3], [1, 5, 9], [0, 5]):
        with pytest.raises(ValueError):
            b.dead_reckon_covariance(take(full, 30, 0), bad_off)
    with pytest.raises(ValueError):
        b.dead_reckon_covariance(take(full, 30, 0), [0, 5, 9], cin)


def test_host_window_form_matches_batch(ctx):
    from cerberus_amd import api
    ws = [kind_window("L70", 1).twin(), frames_window(2).twin(), kind_window("F6", 1).twin()]
    smp, off = _pack([take(w, n, 5 * i) for i, (w, n) in enumerate(zip(ws, (30, 30, 1)))])
    cin = np.array([given_cov(30 + i) for i in range(3)])
    for f, c in ((-1, cin), (1, None), (4, cin)):
        r = api.Batch(ctx, [w.twin() for w in ws]).dead_reckon_covariance(smp, off, c, f, pose_trajectory=True)
        tw = [w.twin() for w in ws]
        h = ctx.window_dead_reckon_covariance(tw, smp, off, c, f, pose_trajectory=True)
        assert list(h.status) == [OK, NO_FRAME if f == 4 else OK, OK]
        for i in range(3):
            _bitwise(_part(h, i), _part(r, i))
            for x, y in zip(tw[i].state_arrays(), ws[i].state_arrays()):
                assert x.tobytes() == y.tobytes()
    # USE_LEG = 0 through the host form (a batch of its own: one IMU factor kind per batch)
    imu = kind_window("L9", 0)
    a, o = _pack([take(imu, 30, 1)])
    _bitwise(_part(ctx.window_dead_reckon_covariance([imu.twin()], a, o), 0), _part(api.Batch(ctx, [imu.twin()]).dead_reckon_covariance(a, o), 0))


def test_bad_arguments(ctx, cfg):
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    w = kind_window("L9", 1).twin()
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_dead_reckon_covariance
    smp, off = _pack([take(w, 30, 0)])
    cin = given_cov(40)[None].copy()
    st, cv, tr, rec = np.zeros((1, 10)), np.zeros((1, 15, 15)), np.zeros((29, 6, 6)), (T.WindowDeadReckonRecord * 1)()
    ps, po = C.cast(smp.ctypes.data, C.POINTER(T.Sample)), T.iptr(off)
    pci, pst, pcv, ptr = (x.ctypes.data_as(T.c_double_p) for x in (cin, st, cv, tr))

    def opts(**kw):
        o = T.DrCovOpts()
        api.lib().vilo_default_dr_cov_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    assert f(None, b.handle, opts(), ps, po, pci, pst, pcv, ptr, rec) == -2
    assert f(ctx.h, None, opts(), ps, po, pci, pst, pcv, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(), ps, None, pci, pst, pcv, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(), ps, po, pci, None, pcv, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(), ps, po, pci, pst, None, ptr, rec) == -2          # NULL cov_out with windows present
    assert b"cov_out" in api.lib().vilo_last_error(ctx.h)
    assert f(ctx.h, b.handle, opts(), None, po, pci, pst, pcv, ptr, rec) == -2         # NULL samples with samples to read
    for bad in (-2, T.MAX_FRAMES):
        assert f(ctx.h, b.handle, opts(from_frame=bad), ps, po, pci, pst, pcv, ptr, rec) == -2
    assert b"from_frame" in api.lib().vilo_last_error(ctx.h)
    assert f(ctx.h, b.handle, opts(reserved=1), ps, po, pci, pst, pcv, ptr, rec) == -2
    for bad in ([1, 30], [0, -1], [30, 0]):
        bo = np.array(bad, np.int32)
        assert f(ctx.h, b.handle, opts(), ps, T.iptr(bo), pci, pst, pcv, ptr, rec) == -2
    g = api.lib().vilo_window_dead_reckon_covariance
    ds, ss = w.desc(T)
    assert g(ctx.h, 0, C.byref(ds), C.byref(ss), opts(), ps, po, pci, pst, pcv, ptr, rec) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(from_frame=11), ps, po, pci, pst, pcv, ptr, rec) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(), ps, po, pci, pst, None, ptr, rec) == -2
    assert not st.any() and not cv.any() and not tr.any() and rec[0].n_steps == 0 and rec[0].status == 0
    assert cin.tobytes() == given_cov(40)[None].tobytes()
    # the batch is still usable; NULL options are the defaults; cov_in, the trajectory and the records may be left out; no samples at all
    assert f(ctx.h, b.handle, None, ps, po, None, pst, pcv, None, None) == 0
    r = b.dead_reckon_covariance(smp, off, None, pose_trajectory=True)
    assert st.tobytes() == r.state.tobytes() and cv.tobytes() == r.cov.tobytes() and r.status[0] == OK and not tr.any()
    assert api.lib().vilo_last_dr_cov_ms(ctx.h) > 0.0
    assert f(ctx.h, b.handle, opts(), ps, po, pci, pst, pcv, ptr, rec) == 0 and (rec[0].status, rec[0].n_steps) == (OK, 29)
    r = b.dead_reckon_covariance(smp, off, cin, pose_trajectory=True)
    assert tr.tobytes() == r.pose_cov_trajectory.tobytes() and cv.tobytes() == r.cov.tobytes()
    zero = np.zeros(2, np.int32)
    assert f(ctx.h, b.handle, opts(), None, T.iptr(zero), pci, pst, pcv, ptr, rec) == 0 and (rec[0].status, rec[0].n_steps) == (OK, 0)
    assert cv.tobytes() == DC.mirrored(cin[0]).tobytes()   # no step: the mirrored input
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), None, ps, po, pci, pst, pcv, ptr, rec) == 0 and cv.tobytes() == r.cov.tobytes()
    _check_parity(r, 0, w, take(w, 30, 0), cfg.g_norm, DC.noise_of(cfg), -1, cin[0], "after bad arguments")
