"""GPU (-m gpu): vilo_batch_leg_dead_reckon / vilo_window_leg_dead_reckon against the numpy definition (tests/leg_dr_model.py) at the state
the device holds. Shapes: batches of 1, 3, 17 and 65 windows (k_leg_dead_reckon gives a window four lanes, a wave sixteen windows, a
workgroup 64: window 17 is the first of a second wave, window 65 of a second workgroup); ranges of 0, 1, 2, 3 and 12 samples side by side;
from_frame -1 and an explicit frame; windows of 2 and 11 frames in one batch (NO_FRAME beside OK); contact models 0, 1 and 2, each with
its own context; the three branch inputs of tests/test_leg_dead_reckon.py. Tolerance: ten times the FP64 floor that file measures
(leg_dr_model.TOL); the flags, n_steps and statuses exactly."""
import ctypes as C

import numpy as np
import pytest

import leg_dr_model as L
from test_covariance_gpu import _window
from test_dead_reckon import frames_window, take
from test_gyro_align import kind_window
from test_leg_dead_reckon import EXPLICIT, MODELS, RANGES, branch_cases, check_against_definition, for_model, model_cfg

pytestmark = pytest.mark.gpu

OK, NO_FRAME, NUMERIC = L.OK, L.NO_FRAME, L.NUMERIC


@pytest.fixture(scope="module")
def ctxs():
    from cerberus_amd import api
    c = {m: api.Context(model_cfg(m), 0) for m in MODELS}
    yield c
    for x in c.values():
        x.close()


def _pack(ranges):
    off = np.zeros(len(ranges) + 1, np.int32)
    off[1:] = np.cumsum([len(r) for r in ranges])
    return np.ascontiguousarray(np.concatenate([np.reshape(r, (-1, 35)) for r in ranges])), off


def _part(r, i):
    """window i's outputs, every array of them"""
    out = [np.ascontiguousarray(r.state[i]), np.ascontiguousarray(r.legs[i]), np.asarray(r.n_steps[i]), np.asarray(r.status[i])]
    if r.trajectory is not None:
        out.append(np.ascontiguousarray(r.trajectory[r.step_offsets[i]:r.step_offsets[i + 1]]))
    return out


def _bitwise(x, y):
    for a, b in zip(x, y):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert a.tobytes() == b.tobytes()


def subjects(m):
    """(window, samples) the batches of contact model m are made of: an 11-frame window at every range length, the 2-frame window, and
    the branch inputs of the model"""
    w, two = kind_window("L9", 1), frames_window(2)
    out = [(w, for_model(take(w, n, 5 * i + 2), m, i)) for i, n in enumerate(RANGES)]
    out.append((two, for_model(take(two, 12, 3), m, 5)))
    out += [(bw, s) for _, bm, bw, s, _, _ in branch_cases() if bm == m]
    return out


def _check(r, i, ref, tag, worst):
    t = r.trajectory[r.step_offsets[i]:r.step_offsets[i + 1]]
    check_against_definition(tag, (r.status[i], r.n_steps[i], r.state[i], r.legs[i], t), ref, worst)
    if ref.status == OK and ref.n_steps:
        # a window's last trajectory row is its state_out, bit for bit
        assert t[-1, 0:4].tobytes() == np.concatenate([r.state[i, 0:1], r.state[i, 23:26]]).tobytes() and t[-1, 7:11].tobytes() == r.state[i, 26:30].tobytes(), tag
    if ref.status != OK:
        assert not r.state[i].any() and not r.legs[i].any() and not t.any(), tag


@pytest.mark.parametrize("m", MODELS)
def test_parity_with_numpy_at_every_batch_size(ctxs, m):
    """batches of 1, 3, 17 and 65 windows made of the model's subjects in turn, from the last frame and from an explicit one (the 2-frame
    window then has no such frame), with and without the trajectory (the same state bits)"""
    from cerberus_amd import api
    subj = subjects(m)
    refs, worst = {}, {}
    for W in (1, 3, 17, 65):
        pick = [(k + W) % len(subj) for k in range(W)]
        ws = [subj[k][0].twin() for k in pick]
        samples, offsets = _pack([subj[k][1] for k in pick])
        b = api.Batch(ctxs[m], ws)
        for f in (-1, EXPLICIT):
            r = b.leg_dead_reckon(samples, offsets, f, trajectory=True)
            assert r.trajectory.shape == (r.step_offsets[-1], L.TRAJ) and r.legs.shape == (W, 4, 3)
            for i, k in enumerate(pick):
                if (k, f) not in refs:
                    refs[(k, f)] = L.window_leg_dead_reckon(model_cfg(m), subj[k][0], subj[k][1], f)
                assert refs[(k, f)].status == (NO_FRAME if f >= subj[k][0].F else OK)
                _check(r, i, refs[(k, f)], "model %d, %d windows, window %d (subject %d), from_frame %d" % (m, W, i, k, f), worst)
            r0 = b.leg_dead_reckon(samples, offsets, f)
            assert r0.trajectory is None and r0.state.tobytes() == r.state.tobytes() and r0.legs.tobytes() == r.legs.tobytes()
            assert r0.status.tobytes() == r.status.tobytes() and r0.n_steps.tobytes() == r.n_steps.tobytes()
        if W == 65:
            assert NO_FRAME in r.status and OK in r.status
    print("MEASURED model %d against the definition: %s (floor %.0e, tolerance %.0e)"
          % (m, ", ".join("%s %.1e" % kv for kv in sorted(worst.items())), L.FLOOR, L.TOL))


@pytest.mark.parametrize("m", MODELS)
def test_independent_of_batch_size_and_position(ctxs, m):
    """every window of the 65-window batch, solved alone in a batch of one, and at another position of the batch in reversed order:
    bit for bit the same outputs"""
    from cerberus_amd import api
    subj = subjects(m)
    pick = [(k + 65) % len(subj) for k in range(65)]

    def run(order):
        smp, off = _pack([subj[k][1] for k in order])
        return api.Batch(ctxs[m], [subj[k][0].twin() for k in order]).leg_dead_reckon(smp, off, -1, trajectory=True)
    full, rev = run(pick), run(pick[::-1])
    for i in range(65):
        _bitwise(_part(full, i), _part(rev, 64 - i))
    for i in (0, 15, 16, 17, 63, 64):
        _bitwise(_part(full, i), _part(run([pick[i]]), 0))


@pytest.mark.parametrize("m", MODELS)
def test_agrees_with_preintegrate(ctxs, m):
    """delta_q, delta_v, delta_eps and sum_dt against Context.preintegrate on the same samples at the state's biases, within the tolerance.
    (Not bit for bit: kernels_preint.hip contracts multiply-adds inside an expression, kernels_legdr.hip rounds every operation.)"""
    from cerberus_amd import api
    subj = [(w, s) for w, s in subjects(m) if len(s) >= 2 and w.F == 11]
    smp, off = _pack([s for _, s in subj])
    ws = [w.twin() for w, _ in subj]
    worst, same = 0.0, 0
    for f in (-1, EXPLICIT):
        r = api.Batch(ctxs[m], ws).leg_dead_reckon(smp, off, f)
        lin = np.array([np.concatenate([w.speed_bias[f, 3:9], w.leg_bias[f]]) for w in ws])
        pre = ctxs[m].preintegrate(smp, off, lin)
        for i in range(len(ws)):
            assert r.status[i] == OK
            got, ref = r.state[i, 0:20], np.concatenate([pre[i, 0:1], pre[i, 4:8], pre[i, 8:11], pre[i, 11:23]])
            e = max(L._err(got[0:1], ref[0:1]), L._err(got[1:5], ref[1:5]), L._err(got[5:8], ref[5:8]), L._err(got[8:20], ref[8:20]))
            worst = max(worst, e)
            same += got.tobytes() == ref.tobytes()
    print("MEASURED model %d against vilo_preintegrate: %.1e (tolerance %.0e); bit for bit in %d of %d" % (m, worst, L.TOL, same, 2 * len(ws)))
    assert worst <= L.TOL


def _state(ws):
    return [a.copy() for w in ws for a in w.state_arrays()]


def _sequence(ctx, base, opts, report):
    from cerberus_amd import api
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    b.solve(opts)
    summ0 = b.download()
    before = _state(ws)
    if report:
        smp, off = _pack([take(w, 12, 4 * i) for i, w in enumerate(ws)])
        bytes0, path0 = b.device_bytes(), b.path()
        first = b.leg_dead_reckon(smp, off, trajectory=True)
        assert b.device_bytes() == bytes0   # nothing is kept with the batch: not even at the first call
        for f in (-1, 3):
            r = b.leg_dead_reckon(smp, off, f, trajectory=(f == -1))
            assert b.device_bytes() == bytes0 and list(r.status) == [OK] * len(ws)
        _bitwise(_part(first, 1), _part(b.leg_dead_reckon(smp, off, trajectory=True), 1))
        assert b.path() == path0
        summ1 = b.download()
        for x, y in zip(before, _state(ws)):
            assert x.tobytes() == y.tobytes()
        assert [bytes(s) for s in summ0] == [bytes(s) for s in summ1]
    b.solve(opts)
    replay = b.path()["replay"]
    summ = b.download()
    return _state(ws), [bytes(s) for s in summ], replay


def test_no_side_effects(ctxs, cfg, ocfg):
    """solve, leg-dead-reckon, download: states, summaries and path() bit for bit unchanged and device_bytes() where it was; the solve
    that follows (a replay of the captured graph) is bit for bit what it is without the calls"""
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s, L=60) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)
    st_a, su_a, rp_a = _sequence(ctxs[0], base, opts, False)
    st_b, su_b, rp_b = _sequence(ctxs[0], base, opts, True)
    for x, y in zip(st_a, st_b):
        assert x.tobytes() == y.tobytes()
    assert su_a == su_b and rp_a == rp_b and rp_b


@pytest.mark.parametrize("m", (0, 2))
def test_not_finite_fails_one_window_alone(ctxs, m):
    """a NaN in one window's start state (a gyro bias, a leg bias) or in one of its samples (a joint velocity): NUMERIC there alone, zero
    rows; its neighbours are bit for bit what they are alone"""
    from cerberus_amd import api
    full = kind_window("L9", 1)
    rs0 = [for_model(take(full, 12, 0), m, 1), for_model(take(full, 12, 3), m, 2), for_model(take(full, 3, 20), m, 3)]

    def alone(w, s):
        a, o = _pack([s])
        return _part(api.Batch(ctxs[m], [w.twin()]).leg_dead_reckon(a, o, 5, trajectory=True), 0)
    for kind in ("bias", "leg_bias", "sample"):
        ws = [full.twin(), full.twin(), full.twin()]
        rs = [r.copy() for r in rs0]
        if kind == "bias":
            ws[1].speed_bias[5, 7] = np.nan
        elif kind == "leg_bias":
            ws[1].leg_bias[5, 2] = np.nan
        else:
            rs[1][7, 19 + 4] = np.nan
        a, o = _pack(rs)
        r = api.Batch(ctxs[m], ws).leg_dead_reckon(a, o, 5, trajectory=True)
        assert list(r.status) == [OK, NUMERIC, OK] and list(r.n_steps) == [11, 11, 2], kind
        ref = L.window_leg_dead_reckon(model_cfg(m), ws[1], rs[1], 5)
        assert ref.status == NUMERIC
        _check(r, 1, ref, "NaN in a %s" % kind, {})
        for i in (0, 2):
            _bitwise(_part(r, i), alone(full, rs[i]))
    # the same NaN in another frame's bias, in the velocity of frame 5, or in a sample no range reads, fails nothing
    w = full.twin()
    w.speed_bias[6, 7] = np.nan
    w.speed_bias[5, 1] = np.nan
    a, o = _pack([rs0[0]])
    assert api.Batch(ctxs[m], [w]).leg_dead_reckon(a, o, 5).status[0] == OK


def test_host_window_form_matches_batch(ctxs):
    from cerberus_amd import api
    ws = [kind_window("L70", 1).twin(), frames_window(2).twin(), kind_window("F6", 1).twin()]
    smp, off = _pack([take(w, n, 5 * i) for i, (w, n) in enumerate(zip(ws, (12, 12, 1)))])
    for f in (-1, 3):
        r = api.Batch(ctxs[0], [w.twin() for w in ws]).leg_dead_reckon(smp, off, f, trajectory=True)
        tw = [w.twin() for w in ws]
        h = ctxs[0].window_leg_dead_reckon(tw, smp, off, f, trajectory=True)
        assert list(h.status) == [OK, NO_FRAME if f == 3 else OK, OK]
        for i in range(3):
            _bitwise(_part(h, i), _part(r, i))
            for x, y in zip(tw[i].state_arrays(), ws[i].state_arrays()):
                assert x.tobytes() == y.tobytes()


def test_bad_arguments_and_unsupported(ctxs):
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    ctx = ctxs[0]
    w = kind_window("L9", 1).twin()
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_leg_dead_reckon
    smp, off = _pack([take(w, 12, 0)])
    st, lg, tr, rec = np.zeros((1, 32)), np.zeros((1, 12)), np.zeros((11, 48)), (T.WindowLegDeadReckonRecord * 1)()
    ps, po = C.cast(smp.ctypes.data, C.POINTER(T.Sample)), T.iptr(off)
    pst, plg, ptr = st.ctypes.data_as(T.c_double_p), lg.ctypes.data_as(T.c_double_p), tr.ctypes.data_as(T.c_double_p)

    def opts(**kw):
        o = T.LegDeadReckonOpts()
        api.lib().vilo_default_leg_dead_reckon_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    assert f(None, b.handle, opts(), ps, po, pst, plg, ptr, rec) == -2
    assert f(ctx.h, None, opts(), ps, po, pst, plg, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(), ps, None, pst, plg, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(), ps, po, None, plg, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(), ps, po, pst, None, ptr, rec) == -2
    assert f(ctx.h, b.handle, opts(), None, po, pst, plg, ptr, rec) == -2          # NULL samples with samples to read
    for bad in (-2, T.MAX_FRAMES):
        assert f(ctx.h, b.handle, opts(from_frame=bad), ps, po, pst, plg, ptr, rec) == -2
    assert b"from_frame" in api.lib().vilo_last_error(ctx.h)
    assert f(ctx.h, b.handle, opts(reserved=1), ps, po, pst, plg, ptr, rec) == -2
    for bad in ([1, 12], [0, -1], [12, 0]):
        bo = np.array(bad, np.int32)
        assert f(ctx.h, b.handle, opts(), ps, T.iptr(bo), pst, plg, ptr, rec) == -2
    g = api.lib().vilo_window_leg_dead_reckon
    ds, ss = w.desc(T)
    assert g(ctx.h, 0, C.byref(ds), C.byref(ss), opts(), ps, po, pst, plg, ptr, rec) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(from_frame=11), ps, po, pst, plg, ptr, rec) == -2
    # a batch of use_leg == 0 windows: unsupported, nothing written
    imu = kind_window("L9", 0).twin()
    bi = api.Batch(ctx, [imu])
    assert f(ctx.h, bi.handle, opts(), ps, po, pst, plg, ptr, rec) == -5
    assert b"use_leg" in api.lib().vilo_last_error(ctx.h)
    with pytest.raises(api.ViloError):
        bi.leg_dead_reckon(smp, off)
    di, si = imu.desc(T)
    assert g(ctx.h, 1, C.byref(di), C.byref(si), opts(), ps, po, pst, plg, ptr, rec) == -5
    assert not st.any() and not lg.any() and not tr.any() and rec[0].n_steps == 0 and rec[0].status == 0
    # the batch is still usable; NULL options are the defaults, the trajectory and the records may be left out; no samples at all
    assert f(ctx.h, b.handle, None, ps, po, pst, plg, None, None) == 0
    r = b.leg_dead_reckon(smp, off, trajectory=True)
    assert st.tobytes() == r.state.tobytes() and lg.tobytes() == r.legs.tobytes() and r.status[0] == OK and not tr.any()
    assert api.lib().vilo_last_leg_dead_reckon_ms(ctx.h) > 0.0
    assert f(ctx.h, b.handle, opts(), ps, po, pst, plg, ptr, rec) == 0 and (rec[0].status, rec[0].n_steps) == (OK, 11)
    assert tr.tobytes() == r.trajectory.tobytes()
    zero = np.zeros(2, np.int32)
    assert f(ctx.h, b.handle, opts(), None, T.iptr(zero), pst, plg, ptr, rec) == 0 and (rec[0].status, rec[0].n_steps) == (OK, 0)
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), None, ps, po, pst, plg, ptr, rec) == 0 and st.tobytes() == r.state.tobytes()
    with pytest.raises(ValueError):
        b.leg_dead_reckon(smp, [0, 5, 3])
