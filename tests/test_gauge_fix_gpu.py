"""GPU (-m gpu): vilo_batch_gauge_fix / vilo_batch_failure_detection and their host forms. The batch sequence solve + gauge_fix + download
+ marginalize against vilo_optimize_windows, bit for bit; both calls against the numpy definitions (tests/gauge_ref.py) at the state the
device returns, within ten times the FP64 floor tests/test_gauge_fix.py measures, flags and statuses exactly; independence of batch size
and position; the host forms; side effects (what moves, reset, device_bytes, the following solve, constant extrinsics); statuses; the
gauge invariance of the cost. Windows of 11, 6 and 2 frames with at most 24 landmarks."""
import ctypes as C

import numpy as np
import pytest

import alt_config
import gauge_ref as G
from test_gauge_fix import (GG, IMU_GROUP, LEG_GROUP, SOLVED, failure_inputs, failure_windows, given_anchor, golden_windows, shape_window)

pytestmark = pytest.mark.gpu


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


def _state(ws):
    return [a.copy() for w in ws for a in w.state_arrays()]


def _same(x, y):
    assert len(x) == len(y)
    for a, b in zip(x, y):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


def _gauge_part(r, i):
    return [np.asarray(r.yaw_diff_deg[i]), np.asarray(r.singular[i]), np.asarray(r.status[i])] + ([r.pose0_before[i].copy()] if r.pose0_before is not None else [])


def _ex_moved(got, ref):
    """how far extrinsic quaternions [2, 7] are from others, up to the sign Quaterniond(Matrix3d) is free to choose"""
    return max(min(np.abs(g[3:] - r[3:]).max(), np.abs(g[3:] + r[3:]).max()) for g, r in zip(got, ref))


def _failure_part(r, i):
    return [np.asarray(r.flags[i]), np.asarray(r.would_reboot[i]), np.asarray(r.status[i]), r.values[i].copy()]


# ---- against the parent's own path ---------------------------------------------------------------------------------------------------
def test_batch_sequence_equals_optimize_windows(ctx, cfg, ocfg):
    """Batch solve + gauge_fix() + download() + marginalize(modes) against vilo_optimize_windows on the same windows, both marginalisation
    modes present: states and priors bit for bit. (Extrinsics free: on a constant extrinsic block the one call rewrites the quaternions
    normalised and the batch call leaves them, include/vilo_gpu.h.)"""
    from cerberus_amd import api, _ctypes as T
    from cerberus_amd.synth import PriorData
    from test_gpu_parity import _fresh
    opts = api.default_solve_opts(True, 4)
    modes = [0, 1, 0, 1]
    one = [_fresh(cfg, ocfg, n_landmarks=24, seed=80 + i) for i in range(4)]
    seq = [_fresh(cfg, ocfg, n_landmarks=24, seed=80 + i) for i in range(4)]
    W = len(one)
    descs, states, summ, priors = (T.WindowDesc * W)(), (T.WindowState * W)(), (T.SolveSummary * W)(), (T.Prior * W)()
    p_one, p_seq = [PriorData() for _ in one], [PriorData() for _ in seq]
    for i, w in enumerate(one):
        descs[i], states[i] = w.desc(T)
        priors[i] = p_one[i].struct
    ctx._check(api.lib().vilo_optimize_windows(ctx.h, W, descs, states, C.byref(opts), (C.c_int * W)(*modes), priors, summ))
    b = api.Batch(ctx, seq)
    b.solve(opts)
    b.download()
    raw = _state(seq)
    r = b.gauge_fix()
    assert list(r.status) == [G.GAUGE_OK] * W
    b.download()
    b.marginalize(modes, p_seq)
    b.close()
    _same(_state(seq), _state(one))
    assert any(x.tobytes() != y.tobytes() for x, y in zip(_state(seq), raw)), "the fix moved nothing: the comparison shows nothing"
    for i in range(W):
        p_one[i].struct = priors[i]
        assert p_one[i].struct.valid == p_seq[i].struct.valid == 1 and p_one[i].n == p_seq[i].n
        assert p_one[i].blocks() == p_seq[i].blocks()
        n = p_one[i].n
        assert p_one[i].J0[:n * n].tobytes() == p_seq[i].J0[:n * n].tobytes() and p_one[i].r0[:n].tobytes() == p_seq[i].r0[:n].tobytes(), i
        assert p_one[i].x0.tobytes() == p_seq[i].x0.tobytes(), i


# ---- parity ------------------------------------------------------------------------------------------------------------------------
def _check_gauge(b, ws, anchors, tag):
    """gauge_fix on batch b whose windows' arrays hold its device state; anchors [W, 7] or None (uploaded: frame 0 of shape_window);
    returns the largest error, and on how many constant extrinsic blocks a rewrite would have shown (quaternions the normalisation moves
    by 1e-10 or more, far above a rounding: test_gauge_fix.generic_extrinsics)"""
    before = [[a.copy() for a in w.state_arrays()] for w in ws]
    r = b.gauge_fix("uploaded" if anchors is None else "given", anchors, pose0_before=True)
    b.download()
    worst, told = 0.0, 0
    for i, w in enumerate(ws):
        a = w.uploaded_pose0 if anchors is None else anchors[i]
        ref = G.gauge_fix(a, before[i][0][:w.F], before[i][1][:w.F], before[i][3], bool(w.ex_const))
        assert r.status[i] == ref.status == G.GAUGE_OK and r.singular[i] == ref.singular, (tag, i)
        assert r.pose0_before[i].tobytes() == before[i][0][0].tobytes(), (tag, i)
        e = G.gauge_error((w.pose, w.speed_bias, w.ex_pose), (ref.pose, ref.speed_bias, ref.ex_pose), w.F)
        ey = abs(r.yaw_diff_deg[i] - ref.yaw_diff_deg) / 180 if not ref.singular else 0.0
        print("MEASURED gauge fix %s window %d (%d frames, singular %d): %.1e, yaw_diff %.1e (tolerance %.0e)" % (tag, i, w.F, ref.singular, e, ey, G.TOL))
        assert max(e, ey) <= G.TOL, (tag, i, e, ey)
        # nothing but pose, velocity and extrinsic-quaternion entries moves; a constant extrinsic block not at all
        assert w.speed_bias[:, 3:].tobytes() == before[i][1][:, 3:].tobytes() and w.ex_pose[:, :3].tobytes() == before[i][3][:, :3].tobytes()
        assert w.pose[w.F:].tobytes() == before[i][0][w.F:].tobytes() and w.speed_bias[w.F:].tobytes() == before[i][1][w.F:].tobytes()
        for j in (2, 4, 5):
            assert w.state_arrays()[j].tobytes() == before[i][j].tobytes()
        shows = _ex_moved(G.gauge_fix(a, before[i][0][:w.F], before[i][1][:w.F], before[i][3], False).ex_pose, before[i][3]) > 1e-10
        if w.ex_const:
            assert w.ex_pose.tobytes() == before[i][3].tobytes(), (tag, i)
            told += shows
        elif shows:
            assert _ex_moved(w.ex_pose, before[i][3]) > 1e-10, (tag, i)
        worst = max(worst, e, ey)
    return worst, told


def _check_failure(b, ws, tag):
    worst = 0.0
    for shift in (0, 1, 2, 3):
        tracks, last = failure_inputs(ws, shift)
        r = b.failure_detection(tracks, last)
        for i, w in enumerate(ws):
            ref = G.window_failure_detection(w, tracks[i], last[i])
            assert (r.flags[i], r.would_reboot[i], r.status[i]) == (ref.flags, ref.would_reboot, G.FAILURE_OK), (tag, shift, i, r.flags[i], ref.flags)
            e = G.values_error(r.values[i], ref.values)
            assert e <= G.TOL_FAILURE, (tag, shift, i, e)
            worst = max(worst, e)
    # without the caller's arrays: bits 0 and 3 to 5 stay 0, their values 0, the others as with them
    r0 = b.failure_detection()
    assert not (r0.flags & 0b111001).any() and not r0.values[:, [0, 3, 4, 5]].any()
    assert r0.values[:, 1:3].tobytes() == r.values[:, 1:3].tobytes() and ((r0.flags ^ r.flags) & 6 == 0).all()
    print("MEASURED failure detection %s: largest error %.1e (floor %.0e, tolerance %.0e)" % (tag, worst, G.FLOOR_FAILURE, G.TOL_FAILURE))
    return worst


def _twins(names):
    ws = []
    for n in names:
        w = shape_window(n).twin()
        w.uploaded_pose0 = shape_window(n).pose[0].copy()
        ws.append(w)
    return ws


@pytest.mark.parametrize("which", ["default", "alt"])
@pytest.mark.parametrize("group", ["leg", "imu"])
def test_parity_with_numpy(ctx, actx, group, which):
    """IMU-leg windows of 11 (extrinsics free, and one window with generic extrinsic quaternions once constant and once free), 6 and 2
    frames in one batch, an IMU-only window in its own; given anchors at the initial state, uploaded and given anchors after a
    4-iteration solve (windows the solver takes: 11 and 6 frames), under both configurations (no kernel of the two calls reads the
    configuration: it enters through the state the solve reaches); the failure criteria at the initial state (large biases on some last
    frames) and at the solved one. On the constant extrinsic block a rewrite would show at every state, and the block comes back as
    uploaded; its free twin is rewritten."""
    from cerberus_amd import api
    c = actx if which == "alt" else ctx
    names = LEG_GROUP if group == "leg" else IMU_GROUP
    ws = _twins(names)
    b = api.Batch(c, ws)
    anchors = np.array([given_anchor(w.pose[0], k) for k, w in enumerate(ws)])
    worst, told = _check_gauge(b, ws, anchors, "%s %s initial given" % (group, which))
    assert told == sum(w.ex_const for w in ws) == (group == "leg")
    assert group != "leg" or _ex_moved(ws[names.index("F11exfree")].ex_pose, shape_window("F11exfree").ex_pose) > 1e-10
    wf = failure_windows(names, "initial")
    bf = api.Batch(c, wf)
    _check_failure(bf, wf, "%s %s initial" % (group, which))
    bf.close()
    b.close()
    ws = _twins([n for n in names if n in SOLVED])
    b = api.Batch(c, ws)
    opts = api.default_solve_opts(True, 4)
    for anchors in (None, np.array([given_anchor(w.uploaded_pose0, k) for k, w in enumerate(ws)])):
        b.reset()
        b.solve(opts)
        b.download()
        _check_failure(b, ws, "%s %s solved" % (group, which))
        e, told = _check_gauge(b, ws, anchors, "%s %s solved %s" % (group, which, "uploaded" if anchors is None else "given"))
        assert told == (group == "leg")
        worst = max(worst, e)
    b.close()
    print("MEASURED gauge fix %s %s: largest error %.1e (floor %.0e, tolerance %.0e)" % (group, which, worst, G.FLOOR, G.TOL))


def test_parity_at_the_euler_singularity(ctx):
    """the golden's 13 cases as one batch: frame-0 pitch within a degree of +-90 before or after on some, not on others"""
    from cerberus_amd import api
    gw = golden_windows()
    ws = [w.twin() for w, _ in gw]
    anchors = np.array([a for _, a in gw])
    b = api.Batch(ctx, ws)
    before = _state(ws)
    worst, _ = _check_gauge(b, ws, anchors, "golden")
    b.reset()
    r = b.gauge_fix("given", anchors)
    assert list(r.singular) == [int(t) for t in GG["branch_taken"]] and 0 < r.singular.sum() < len(ws)
    b.reset()
    b.download()
    _same(_state(ws), before)   # reset() restores the upload
    b.close()
    print("MEASURED gauge fix at the Euler singularity: largest error %.1e (tolerance %.0e)" % (worst, G.TOL))


# ---- batch size and position ---------------------------------------------------------------------------------------------------------
def test_independent_of_batch_size_and_position(ctx):
    """alone, at position 3 of 8 and at positions 0 / 150 / 299 of 300 windows of mixed shape: both calls bit for bit the same"""
    from cerberus_amd import api
    others = [shape_window("F11"), shape_window("F6"), shape_window("F2")]
    subjects = [(golden_windows()[4][0], golden_windows()[4][1]), (shape_window("F6"), given_anchor(shape_window("F6").pose[0], 2)),
                (shape_window("F2"), given_anchor(shape_window("F2").pose[0], 1))]
    for w, anchor in subjects:
        def run(ws, at):
            anchors = np.array([given_anchor(x.pose[0], i % 5) for i, x in enumerate(ws)])
            for p in at:
                anchors[p] = anchor
            tracks, last = failure_inputs(ws, 1)
            t1, l1 = failure_inputs([w], 1)
            for p in at:
                tracks[p], last[p] = t1[0], l1[0]
            b = api.Batch(ctx, ws)
            f = b.failure_detection(tracks, last)
            g = b.gauge_fix("given", anchors, pose0_before=True)
            b.download()
            b.close()
            return [_failure_part(f, p) + _gauge_part(g, p) + [a.copy() for a in ws[p].state_arrays()] for p in at]
        alone = run([w.twin()], [0])[0]
        assert alone[2] == G.FAILURE_OK and alone[6] == G.GAUGE_OK

        def crowd(n, at):
            ws = [others[i % 3].twin() for i in range(n)]
            for p in at:
                ws[p] = w.twin()
            return run(ws, at)
        for got in crowd(8, [3]) + crowd(300, [0, 150, 299]):
            _same(got, alone)


# ---- forms -------------------------------------------------------------------------------------------------------------------------
def test_host_form_equals_batch_form(ctx):
    from cerberus_amd import api
    names = LEG_GROUP
    wb, wh = _twins(names), _twins(names)
    anchors = np.array([given_anchor(w.pose[0], k) for k, w in enumerate(wb)])
    tracks, last = failure_inputs(wb, 1)
    b = api.Batch(ctx, wb)
    fb, gb = b.failure_detection(tracks, last), b.gauge_fix("given", anchors, pose0_before=True)
    b.download()
    b.close()
    fh = ctx.window_failure_detection(wh, tracks, last)
    gh = ctx.window_gauge_fix(wh, "given", anchors, pose0_before=True)
    for i in range(len(names)):
        _same(_failure_part(fh, i) + _gauge_part(gh, i), _failure_part(fb, i) + _gauge_part(gb, i))
    _same(_state(wh), _state(wb))
    assert any(w.F < 11 for w in wh)   # each window's own n_frames


# ---- side effects ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("replay", [False, True])
def test_gauge_fix_side_effects(ctx, replay):
    """device_bytes() does not move; reset() restores the upload; the solve after the fix (plain launches, and a replay of the captured
    graph) is bit for bit the solve of a batch created at the fixed states; of one window with extrinsic quaternions the normalisation
    moves, the constant block comes back bitwise as uploaded, after the fix and after the solve, and the free twin's is rewritten (what
    else moves and what does not: test_parity_with_numpy)"""
    from cerberus_amd import api
    opts = api.default_solve_opts(True, 4)
    ws = _twins(["F11", "F11ex", "F11exfree", "F6"])
    upload = _state(ws)
    assert ws[1].ex_const and not ws[2].ex_const and upload[6 + 3].tobytes() == upload[12 + 3].tobytes()
    anchors = np.array([given_anchor(w.pose[0], k) for k, w in enumerate(ws)])
    b = api.Batch(ctx, ws)
    if replay:
        b.solve(opts)   # solve once before the fix: the solve after it replays the captured graph
        b.reset()
    bytes0 = b.device_bytes()
    r = b.gauge_fix("given", anchors, pose0_before=True)
    assert b.device_bytes() == bytes0 and list(r.status) == [0, 0, 0, 0]
    assert api.lib().vilo_last_gauge_fix_ms(ctx.h) > 0
    b.download()
    fixed = _state(ws)
    assert ws[1].ex_pose.tobytes() == upload[6 + 3].tobytes()   # the constant extrinsic block, bitwise as uploaded
    assert 1e-10 < _ex_moved(ws[2].ex_pose, upload[12 + 3]) < 1e-8 and ws[2].ex_pose[:, :3].tobytes() == upload[12 + 3][:, :3].tobytes()   # its free twin: normalised
    fresh = [w.twin() for w in ws]
    b.solve(opts)
    s1 = [(s.final_cost, s.iterations) for s in b.download()]
    assert b.path()["replay"] == replay
    b2 = api.Batch(ctx, fresh)
    b2.solve(opts)
    s2 = [(s.final_cost, s.iterations) for s in b2.download()]
    b2.close()
    _same(_state(ws), _state(fresh))
    assert s1 == s2 and ws[1].ex_pose.tobytes() == upload[6 + 3].tobytes()
    assert any(x.tobytes() != y.tobytes() for x, y in zip(_state(ws), fixed))
    b.reset()
    b.download()
    _same(_state(ws), upload)
    b.close()


def test_failure_detection_no_side_effects(ctx):
    """solve, failure_detection, download: states and summaries bit for bit what they are without the call, device_bytes() where it was,
    and the solve that follows (a replay of the captured graph) too"""
    from cerberus_amd import api
    opts = api.default_solve_opts(True, 4)

    def sequence(call):
        ws = _twins(["F11", "F6", "F11ex"])
        b = api.Batch(ctx, ws)
        b.solve(opts)
        if call:
            n0 = b.device_bytes()
            tracks, last = failure_inputs(ws, 1)
            r = b.failure_detection(tracks, last)
            assert b.device_bytes() == n0 and list(r.status) == [0, 0, 0] and api.lib().vilo_last_failure_detection_ms(ctx.h) > 0
        su = [(s.final_cost, s.iterations, s.termination) for s in b.download()]
        st = _state(ws)
        b.reset()
        b.solve(opts)
        if call:
            b.failure_detection()
        su += [(s.final_cost, s.iterations, s.termination) for s in b.download()]
        rp = b.path()["replay"]
        b.close()
        return st + _state(ws), su, rp
    st_a, su_a, rp_a = sequence(False)
    st_b, su_b, rp_b = sequence(True)
    _same(st_a, st_b)
    assert su_a == su_b and rp_a == rp_b and rp_b


# ---- statuses ----------------------------------------------------------------------------------------------------------------------
def test_statuses(ctx):
    """a NaN in one window's frame-0 pose: NUMERIC for the gauge fix of that window, which is left unwritten; a NaN in a last frame's
    gyroscope bias: NUMERIC for the failure detection; the neighbours bit for bit what they are alone. An extrinsic quaternion is read
    only where it would be rewritten: a NaN in a constant block leaves the window VILO_GAUGE_OK and fixed as without it, in its free
    twin's it is NUMERIC"""
    from cerberus_amd import api
    names = ["F11", "F6", "F11", "F2"]
    ws = _twins(names)
    ws[2].pose[0, 4] = np.nan
    ws[1].speed_bias[ws[1].F - 1, 7] = np.nan
    anchors = np.array([given_anchor(shape_window(n).pose[0], k) for k, n in enumerate(names)])
    tracks, last = failure_inputs(_twins(names), 1)
    upload = _state(ws)
    b = api.Batch(ctx, ws)
    f = b.failure_detection(tracks, last)
    g = b.gauge_fix("given", anchors, pose0_before=True)
    b.download()
    b.close()
    assert list(g.status) == [0, 0, G.GAUGE_NUMERIC, 0] and g.yaw_diff_deg[2] == 0 and g.singular[2] == 0
    assert list(f.status) == [0, G.FAILURE_NUMERIC, 0, 0] and f.flags[1] == 0 and f.would_reboot[1] == 0 and not f.values[1].any()
    got = _state(ws)
    for j in range(6):
        assert got[12 + j].tobytes() == upload[12 + j].tobytes()   # the NUMERIC window: nothing written
    for i in (0, 1, 3):
        w1 = _twins([names[i]])
        if i == 1:
            w1[0].speed_bias[w1[0].F - 1, 7] = np.nan
        b1 = api.Batch(ctx, w1)
        f1 = b1.failure_detection(tracks[i:i + 1], last[i:i + 1])
        g1 = b1.gauge_fix("given", anchors[i:i + 1], pose0_before=True)
        b1.download()
        b1.close()
        _same(_failure_part(f, i) + _gauge_part(g, i) + got[6 * i:6 * i + 6], _failure_part(f1, 0) + _gauge_part(g1, 0) + _state(w1))
    # the anchor too is a value read
    ws = _twins(["F6"])
    bad = anchors[1:2].copy()
    bad[0, 0] = np.inf
    b = api.Batch(ctx, ws)
    assert list(b.gauge_fix("given", bad).status) == [G.GAUGE_NUMERIC]
    b.close()
    # a constant extrinsic block is not read
    names = ["F11ex", "F11exfree", "F11ex"]
    ws = _twins(names)
    ws[0].ex_pose[1, 5] = ws[1].ex_pose[1, 5] = np.nan
    upload = _state(ws)
    anchors = np.array([given_anchor(shape_window(n).pose[0], 2) for n in names])
    b = api.Batch(ctx, ws)
    g = b.gauge_fix("given", anchors)
    b.download()
    b.close()
    got = _state(ws)
    assert list(g.status) == [G.GAUGE_OK, G.GAUGE_NUMERIC, G.GAUGE_OK] and g.yaw_diff_deg[0] == g.yaw_diff_deg[2] != 0
    _same(got[0:3] + got[4:6], got[12:15] + got[16:18])          # fixed as the window without the NaN
    assert got[3].tobytes() == upload[3].tobytes() and got[15].tobytes() == upload[15].tobytes()
    assert any(x.tobytes() != y.tobytes() for x, y in zip(got[0:2], upload[0:2]))
    _same(got[6:12], upload[6:12])                               # the NUMERIC window: nothing written


def test_bad_arguments(ctx):
    from cerberus_amd import api, _ctypes as T
    ws = _twins(["F6"])
    b = api.Batch(ctx, ws)
    L = api.lib()
    o = T.GaugeOpts()
    pose = np.zeros((1, 7))
    rec = (T.WindowGaugeRecord * 1)()
    o.anchor = 1
    assert L.vilo_batch_gauge_fix(ctx.h, b.handle, C.byref(o), None, rec, None) != 0            # GIVEN without a pointer
    o.anchor = 0
    assert L.vilo_batch_gauge_fix(ctx.h, b.handle, C.byref(o), api._p(pose), rec, None) != 0    # a pointer without GIVEN
    o.anchor = 7
    assert L.vilo_batch_gauge_fix(ctx.h, b.handle, C.byref(o), None, rec, None) != 0
    assert L.vilo_batch_gauge_fix(ctx.h, None, None, None, rec, None) != 0
    assert L.vilo_batch_failure_detection(ctx.h, b.handle, None, None, None, None) != 0          # no records
    b.download()
    _same(_state(ws), _state(_twins(["F6"])))
    b.close()


# ---- consistency -------------------------------------------------------------------------------------------------------------------
def test_cost_is_gauge_invariant(ctx):
    """after gauge_fix, residuals().cost is what it was before the call, within the bound tests/test_residuals_gpu.py holds between the
    cost and final_cost (1e-12 relative). The anchors are given ones 0.4 and 0.5 rad of yaw and metres away from the uploaded frame 0,
    so the fix turns and shifts the windows by that much: an identity would show nothing."""
    from cerberus_amd import api
    ws = _twins(["F11", "F6"])
    ws[0].prior = ws[0].prior.copy()
    ws[0].prior.struct.valid = 0   # (a prior holds the poses it was linearised at: only the factors' cost is gauge-invariant)
    b = api.Batch(ctx, ws)
    b.solve(api.default_solve_opts(True, 4))
    c0 = b.residuals().cost.copy()
    b.download()
    solved = _state(ws)
    anchors = np.array([given_anchor(w.uploaded_pose0, k) for k, w in enumerate(ws)])
    r = b.gauge_fix("given", anchors, pose0_before=True)
    c1 = b.residuals().cost.copy()
    b.download()
    b.close()
    assert list(r.status) == [0, 0] and list(r.singular) == [0, 0]
    for i, w in enumerate(ws):
        # the fix moved the state: a yaw of more than 10 degrees, every frame more than a quarter of a metre
        assert abs(r.yaw_diff_deg[i]) > 10 and np.abs(w.pose[:w.F, :3] - solved[6 * i][:w.F, :3]).max(axis=1).min() > 0.25, (i, r.yaw_diff_deg[i])
    for i in range(2):
        print("MEASURED cost before / after the gauge fix, window %d: %.15g / %.15g (relative %.1e, bound 1e-12), yaw_diff %.3e deg"
              % (i, c0[i], c1[i], abs(c1[i] - c0[i]) / abs(c0[i]), r.yaw_diff_deg[i]))
        assert abs(c1[i] - c0[i]) <= 1e-12 * abs(c0[i])
