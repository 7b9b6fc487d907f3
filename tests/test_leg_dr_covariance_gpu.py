"""GPU (-m gpu): vilo_batch_leg_dead_reckon_covariance / vilo_window_leg_dead_reckon_covariance against the numpy definition
(tests/leg_dr_cov_ref.py) at the state the device holds. Shapes: batches of 1, 3 and 7 windows (k_leg_dr_covariance gives a window 32
lanes, a wave and a workgroup two windows: window 2 of a batch of 3 is the first of a second wave and of a second workgroup); ranges of
0, 1, 2, 3 and 12 samples side by side; from_frame -1 and 4; windows of 2 and 11 frames in one batch (NO_FRAME beside OK); contact models
0, 1 and 2, each with its own context; the three branch inputs; cov_in NULL, given, and cut from Batch.covariance() after a short solve.
Tolerance: ten times the FP64 floor tests/test_leg_dr_covariance.py measures (leg_dr_cov_ref.TOL); n_steps and statuses exactly."""
import ctypes as C

import numpy as np
import pytest

import leg_dr_cov_ref as R
import leg_dr_model as L
from test_covariance_gpu import _window
from test_dead_reckon import frames_window, take
from test_gyro_align import kind_window
from test_leg_dead_reckon import EXPLICIT, MODELS, for_model
from test_leg_dead_reckon_gpu import _bitwise, _pack, _state, subjects
from test_leg_dr_covariance import cov_cfg, solved_blocks, spd19

pytestmark = pytest.mark.gpu

OK, NO_FRAME, NUMERIC = L.OK, L.NO_FRAME, L.NUMERIC
SIZES = (1, 3, 7)


@pytest.fixture(scope="module")
def ctxs():
    from cerberus_amd import api
    c = {m: api.Context(cov_cfg(m), 0) for m in MODELS}
    yield c
    for x in c.values():
        x.close()


def _part(r, i):
    """window i's outputs, every array of them"""
    a, b = r.step_offsets[i], r.step_offsets[i + 1]
    out = [np.ascontiguousarray(r.state[i]), np.ascontiguousarray(r.legs[i]), np.ascontiguousarray(r.cov[i]), np.asarray(r.n_steps[i]), np.asarray(r.status[i])]
    if r.pose_cov_trajectory is not None:
        out.append(np.ascontiguousarray(r.pose_cov_trajectory[a:b]))
    if r.leg_cov_trajectory is not None:
        out.append(np.ascontiguousarray(r.leg_cov_trajectory[a:b]))
    return out


def _check(r, i, ref, tag):
    """window i of a call with both trajectories against the definition; returns the error"""
    a, b = r.step_offsets[i], r.step_offsets[i + 1]
    cov, pt, lt = r.cov[i], r.pose_cov_trajectory[a:b], r.leg_cov_trajectory[a:b]
    assert (r.status[i], r.n_steps[i]) == (ref.status, ref.n_steps), tag
    assert cov.tobytes() == np.ascontiguousarray(cov.T).tobytes(), tag   # bitwise symmetric
    if ref.status != OK:
        assert not r.state[i].any() and not r.legs[i].any() and not cov.any() and not pt.any() and not lt.any(), tag
        return 0.0
    if ref.n_steps == 0:
        assert cov.tobytes() == ref.cov.tobytes(), tag   # Sigma_0, bit for bit
        return 0.0
    # a window's last trajectory rows are the blocks of its cov_out, bit for bit
    assert pt[-1].tobytes() == np.ascontiguousarray(cov[0:6, 0:6]).tobytes(), tag
    for j in range(4):
        assert lt[-1, j].tobytes() == np.ascontiguousarray(cov[9 + 3 * j:12 + 3 * j, 9 + 3 * j:12 + 3 * j]).tobytes(), tag
    assert np.linalg.eigvalsh(cov).min() >= -R.FLOOR * np.trace(cov), tag
    e = R.cov_error((cov, pt, lt), (ref.cov, ref.pose_cov_trajectory, ref.leg_cov_trajectory))
    assert e <= R.TOL, (tag, e)
    return e


@pytest.mark.parametrize("m", MODELS)
def test_parity_with_numpy_at_every_batch_size(ctxs, m):
    """batches of 1 and 3 windows made of the model's subjects in turn and one of all its subjects (7 or 8), from the last frame and from frame 4 (the 2-frame window then
    has no such frame), cov_in NULL and given; state_out / legs_out bit for bit leg_dead_reckon's; with and without the trajectories"""
    from cerberus_amd import api
    subj = subjects(m)
    refs, worst = {}, 0.0
    for W in SIZES:
        pick = [(k + W) % len(subj) for k in range(W)] if W < 7 else list(range(len(subj)))   # (7 or 8: every subject of the model)
        ws = [subj[k][0].twin() for k in pick]
        samples, offsets = _pack([subj[k][1] for k in pick])
        b = api.Batch(ctxs[m], ws)
        for f in (-1, EXPLICIT):
            for given in (False, True):
                cin = np.array([spd19(k) for k in pick]) if given else None
                r = b.leg_dead_reckon_covariance(samples, offsets, cin, f, pose_trajectory=True, leg_trajectory=True)
                assert r.cov.shape == (len(pick), 31, 31) and r.pose_cov_trajectory.shape == (r.step_offsets[-1], 6, 6) and r.leg_cov_trajectory.shape == (r.step_offsets[-1], 4, 3, 3)
                for i, k in enumerate(pick):
                    if (k, f, given) not in refs:
                        refs[(k, f, given)] = R.window_leg_dr_cov(cov_cfg(m), subj[k][0], subj[k][1], f, spd19(k) if given else None)
                    assert refs[(k, f, given)].status == (NO_FRAME if f >= subj[k][0].F else OK)
                    worst = max(worst, _check(r, i, refs[(k, f, given)], "model %d, %d windows, window %d (subject %d), from_frame %d, cov_in %s" % (m, len(pick), i, k, f, given)))
                n = b.leg_dead_reckon(samples, offsets, f)
                assert n.state.tobytes() == r.state.tobytes() and n.legs.tobytes() == r.legs.tobytes() and n.status.tobytes() == r.status.tobytes() and n.n_steps.tobytes() == r.n_steps.tobytes()
                r0 = b.leg_dead_reckon_covariance(samples, offsets, cin, f)
                assert r0.pose_cov_trajectory is None and r0.leg_cov_trajectory is None
                assert r0.cov.tobytes() == r.cov.tobytes() and r0.state.tobytes() == r.state.tobytes() and r0.status.tobytes() == r.status.tobytes()
    print("MEASURED model %d against the definition: %.2e (floor %.0e, tolerance %.0e)" % (m, worst, R.FLOOR, R.TOL))


@pytest.mark.parametrize("m", MODELS)
def test_independent_of_batch_size_and_position(ctxs, m):
    """every window of a batch against the reversed batch, and a few alone: bit for bit"""
    from cerberus_amd import api
    subj = subjects(m)
    pick = list(range(len(subj)))

    def run(order):
        smp, off = _pack([subj[k][1] for k in order])
        cin = np.array([spd19(k) for k in order])
        return api.Batch(ctxs[m], [subj[k][0].twin() for k in order]).leg_dead_reckon_covariance(smp, off, cin, -1, pose_trajectory=True, leg_trajectory=True)
    full, rev = run(pick), run(pick[::-1])
    n = len(pick)
    for i in range(n):
        _bitwise(_part(full, i), _part(rev, n - 1 - i))
    for i in (0, 1, 2, n - 1):
        _bitwise(_part(full, i), _part(run([pick[i]]), 0))


@pytest.mark.parametrize("m", MODELS)
def test_agrees_with_the_record_formula(ctxs, m):
    """T (Phi Sigma_0' Phi^T + Sigma_rec) T^T from vilo_preintegrate's record of the same samples at the frame's biases"""
    from cerberus_amd import api
    import deadreckon_ref as D
    subj = [(w, s) for w, s in subjects(m) if len(s) >= 2 and w.F == 11]
    smp, off = _pack([s for _, s in subj])
    ws = [w.twin() for w, _ in subj]
    worst = 0.0
    for given in (False, True):
        cin = np.array([spd19(40 + i) for i in range(len(ws))]) if given else None
        r = api.Batch(ctxs[m], ws).leg_dead_reckon_covariance(smp, off, cin, -1)
        lin = np.array([np.concatenate([w.speed_bias[-1, 3:9], w.leg_bias[-1]]) for w in ws])
        pre = ctxs[m].preintegrate(smp, off, lin)
        for i, w in enumerate(ws):
            assert r.status[i] == OK
            R_f = D.quat_R(D.quat_normalized(np.asarray(w.pose[w.F - 1, 3:7], np.float64), np.float64), np.float64)
            want = R.from_record(pre[i], R_f, R.embed(cin[i] if given else None, np.float64))
            e = R._rel(r.cov[i], want)
            worst = max(worst, e)
            assert e <= R.TOL, (m, i, given, e)
    print("MEASURED model %d against the record formula of vilo_preintegrate: %.2e (tolerance %.0e)" % (m, worst, R.TOL))


def _sequence(ctx, base, opts, report):
    from cerberus_amd import api
    import deadreckon_ref as D
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    b.solve(opts)
    summ0 = b.download()
    before = _state(ws)
    if report:
        smp, off = _pack([take(w, 12, 4 * i) for i, w in enumerate(ws)])
        frames, _, cst = b.covariance(gauge="frame0")
        assert not cst.any()
        bytes0, path0 = b.device_bytes(), b.path()
        nf = np.array([w.F for w in ws])
        worst = tie = 0.0
        for k, f in enumerate((-1, 3)):
            cin = api.leg_dr_cov_in(frames, nf, f)
            # the golden blocks the CPU tie reads are these (another build may round a solve differently: not bit for bit)
            np.testing.assert_allclose(cin, solved_blocks()[2 * k:2 * k + 2], rtol=1e-6, atol=1e-12)
            r = b.leg_dead_reckon_covariance(smp, off, cin, f, pose_trajectory=True, leg_trajectory=True)
            assert b.device_bytes() == bytes0 and list(r.status) == [OK] * len(ws)
            lin = np.array([np.concatenate([w.speed_bias[f, 3:9], w.leg_bias[f]]) for w in ws])
            pre = ctx.preintegrate(smp, off, lin)
            for i, w in enumerate(ws):
                worst = max(worst, _check(r, i, R.window_leg_dr_cov(cov_cfg(0), w, smp[off[i]:off[i + 1]], f, cin[i]), "solved window %d from %d" % (i, f)))
                # and the record formula at the solved window's frame block, from vilo_preintegrate's record
                R_f = D.quat_R(D.quat_normalized(np.asarray(w.pose[f, 3:7], np.float64), np.float64), np.float64)
                e = R._rel(r.cov[i], R.from_record(pre[i], R_f, R.embed(cin[i], np.float64)))
                tie = max(tie, e)
                assert e <= R.TOL, (i, f, e)
        print("MEASURED cov_in from Batch.covariance() after a solve: %.2e against the definition, %.2e against the record formula (tolerance %.0e)"
              % (worst, tie, R.TOL))
        assert b.path() == path0
        summ1 = b.download()
        for x, y in zip(before, _state(ws)):
            assert x.tobytes() == y.tobytes()
        assert [bytes(s) for s in summ0] == [bytes(s) for s in summ1]
    b.solve(opts)
    replay = b.path()["replay"]
    summ = b.download()
    return _state(ws), [bytes(s) for s in summ], replay, _mask_in_force(b, ws)


def _mask_in_force(b, ws):
    """the landmark mask in force, read last (or-ing nothing into it)"""
    mask, _ = b.mask_landmarks(mask=np.zeros(sum(w.L for w in ws), np.uint8), combine="or")
    return np.asarray(mask).tobytes()


def test_no_side_effects_and_cov_in_from_a_solve(ctxs, cfg, ocfg):
    """solve, covariance, leg_dead_reckon_covariance with cov_in cut from it, download: states, summaries and path() bit for bit unchanged
    and device_bytes() where it was; the solve that follows (a replay of the captured graph) and the landmark mask are bit for bit what
    they are without the calls"""
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s, L=60) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)

    def plain(ctx):
        ws = [w.twin() for w in base]
        b = api.Batch(ctx, ws)
        b.solve(opts)
        b.download()
        b.covariance(gauge="frame0")
        b.solve(opts)
        replay = b.path()["replay"]
        summ = b.download()
        return _state(ws), [bytes(s) for s in summ], replay, _mask_in_force(b, ws)
    st_a, su_a, rp_a, m_a = plain(ctxs[0])
    st_b, su_b, rp_b, m_b = _sequence(ctxs[0], base, opts, True)
    for x, y in zip(st_a, st_b):
        assert x.tobytes() == y.tobytes()
    assert su_a == su_b and rp_a == rp_b and rp_b
    assert m_a == m_b and len(m_a) == sum(w.L for w in base)


@pytest.mark.parametrize("m", (0, 2))
def test_not_finite_fails_one_window_alone(ctxs, m):
    """a NaN in one window's start state, in one of its samples or in the read triangle of its cov_in: NUMERIC there alone, zero rows; its
    neighbours are bit for bit what they are alone; a NaN below the diagonal changes nothing"""
    from cerberus_amd import api
    full = kind_window("L9", 1)
    rs0 = [for_model(take(full, 12, 0), m, 1), for_model(take(full, 12, 3), m, 2), for_model(take(full, 3, 20), m, 3)]
    cin0 = np.array([spd19(60 + i) for i in range(3)])

    def alone(w, s, c):
        a, o = _pack([s])
        return _part(api.Batch(ctxs[m], [w.twin()]).leg_dead_reckon_covariance(a, o, c[None], 5, pose_trajectory=True, leg_trajectory=True), 0)
    for kind in ("bias", "sample", "cov_in", "below"):
        ws = [full.twin(), full.twin(), full.twin()]
        rs = [r.copy() for r in rs0]
        cin = cin0.copy()
        if kind == "bias":
            ws[1].speed_bias[5, 7] = np.nan
        elif kind == "sample":
            rs[1][7, 19 + 4] = np.nan
        elif kind == "cov_in":
            cin[1, 2, 16] = np.nan
        else:
            cin[1, 16, 2] = np.nan
        a, o = _pack(rs)
        r = api.Batch(ctxs[m], ws).leg_dead_reckon_covariance(a, o, cin, 5, pose_trajectory=True, leg_trajectory=True)
        if kind == "below":
            assert list(r.status) == [OK, OK, OK]
            _bitwise(_part(r, 1), alone(full, rs0[1], cin0[1]))
            continue
        assert list(r.status) == [OK, NUMERIC, OK] and list(r.n_steps) == [11, 11, 2], kind
        assert not any(x.any() for x in _part(r, 1)[:3] + _part(r, 1)[5:]), kind
        for i in (0, 2):
            _bitwise(_part(r, i), alone(full, rs[i], cin[i]))


def test_host_window_form_matches_batch(ctxs):
    ws = [kind_window("L70", 1).twin(), frames_window(2).twin(), kind_window("F6", 1).twin()]
    from cerberus_amd import api
    smp, off = _pack([take(w, n, 5 * i) for i, (w, n) in enumerate(zip(ws, (12, 12, 1)))])
    cin = np.array([spd19(70 + i) for i in range(3)])
    for f in (-1, 3):
        r = api.Batch(ctxs[0], [w.twin() for w in ws]).leg_dead_reckon_covariance(smp, off, cin, f, pose_trajectory=True, leg_trajectory=True)
        tw = [w.twin() for w in ws]
        h = ctxs[0].window_leg_dead_reckon_covariance(tw, smp, off, cin, f, pose_trajectory=True, leg_trajectory=True)
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
    f = api.lib().vilo_batch_leg_dead_reckon_covariance
    smp, off = _pack([take(w, 12, 0)])
    st, lg, cv, pt, lt, rec = np.zeros((1, 32)), np.zeros((1, 12)), np.zeros((1, 31, 31)), np.zeros((11, 6, 6)), np.zeros((11, 4, 3, 3)), (T.WindowLegDeadReckonRecord * 1)()
    ps, po = C.cast(smp.ctypes.data, C.POINTER(T.Sample)), T.iptr(off)
    p = lambda a: a.ctypes.data_as(T.c_double_p)   # noqa: E731
    out = (p(st), p(lg), p(cv), p(pt), p(lt), rec)

    def opts(**kw):
        o = T.LegDrCovOpts()
        api.lib().vilo_default_leg_dr_cov_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    assert f(None, b.handle, opts(), ps, po, None, *out) == -2
    assert f(ctx.h, None, opts(), ps, po, None, *out) == -2
    assert f(ctx.h, b.handle, opts(), ps, None, None, *out) == -2
    assert f(ctx.h, b.handle, opts(), ps, po, None, None, p(lg), p(cv), p(pt), p(lt), rec) == -2
    assert f(ctx.h, b.handle, opts(), ps, po, None, p(st), None, p(cv), p(pt), p(lt), rec) == -2
    assert f(ctx.h, b.handle, opts(), ps, po, None, p(st), p(lg), None, p(pt), p(lt), rec) == -2   # NULL cov_out
    assert b"cov_out" in api.lib().vilo_last_error(ctx.h)
    assert f(ctx.h, b.handle, opts(), None, po, None, *out) == -2
    for bad in (-2, T.MAX_FRAMES):
        assert f(ctx.h, b.handle, opts(from_frame=bad), ps, po, None, *out) == -2
    assert f(ctx.h, b.handle, opts(reserved=1), ps, po, None, *out) == -2
    for bad in ([1, 12], [0, -1], [12, 0]):
        assert f(ctx.h, b.handle, opts(), ps, T.iptr(np.array(bad, np.int32)), None, *out) == -2
    g = api.lib().vilo_window_leg_dead_reckon_covariance
    ds, ss = w.desc(T)
    assert g(ctx.h, 0, C.byref(ds), C.byref(ss), opts(), ps, po, None, *out) == -2
    imu = kind_window("L9", 0).twin()
    bi = api.Batch(ctx, [imu])
    assert f(ctx.h, bi.handle, opts(), ps, po, None, *out) == -5
    assert b"use_leg" in api.lib().vilo_last_error(ctx.h)
    with pytest.raises(api.ViloError):
        bi.leg_dead_reckon_covariance(smp, off)
    assert not st.any() and not lg.any() and not cv.any() and not pt.any() and not lt.any() and rec[0].n_steps == 0 and rec[0].status == 0
    # the batch is still usable; NULL options are the defaults, the trajectories and the records may be left out
    assert f(ctx.h, b.handle, None, ps, po, None, p(st), p(lg), p(cv), None, None, None) == 0
    r = b.leg_dead_reckon_covariance(smp, off, pose_trajectory=True, leg_trajectory=True)
    assert st.tobytes() == r.state.tobytes() and cv.tobytes() == r.cov.tobytes() and r.status[0] == OK and not pt.any()
    assert api.lib().vilo_last_leg_dr_cov_ms(ctx.h) > 0.0
    assert f(ctx.h, b.handle, opts(), ps, po, None, *out) == 0 and (rec[0].status, rec[0].n_steps) == (OK, 11)
    assert pt.tobytes() == r.pose_cov_trajectory.tobytes() and lt.tobytes() == r.leg_cov_trajectory.tobytes()
    zero = np.zeros(2, np.int32)
    assert f(ctx.h, b.handle, opts(), None, T.iptr(zero), None, *out) == 0 and (rec[0].status, rec[0].n_steps) == (OK, 0) and not cv.any()
    with pytest.raises(ValueError):
        b.leg_dead_reckon_covariance(smp, off, np.zeros((1, 15, 15)))
