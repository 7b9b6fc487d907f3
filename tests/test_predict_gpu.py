"""GPU (-m gpu): vilo_batch_predict_next_frame / vilo_window_predict_next_frame against the numpy definition (tests/predict_ref.py) at
the state the device returns: both modes and both cameras on the packing shapes, the ragged field windows and a copy with skew extrinsics;
the given mode on the pose the constant-velocity mode returned; landmarks behind the next camera; landmarks that are not predicted; two-
and three-frame windows; a non-finite window; windows without landmarks; independence of batch size and position; freedom from side
effects; the host form; the call's device memory; bad arguments. Tolerance: ten times the FP64 floor tests/test_predict.py measures
(predict_ref.TOL), flags and counts exactly."""
import ctypes as C
import itertools

import numpy as np
import pytest

import predict_ref
from test_covariance_gpu import _window
from test_landmark_covariance_gpu import _no_landmarks
from test_predict import FIELD, MODES, Z_CLEAR, field_window, given_pose, skew_extrinsics
from test_triangulate import SHAPES, shape_window

pytestmark = pytest.mark.gpu

OK, TOO_FEW, NUMERIC = predict_ref.OK, predict_ref.TOO_FEW_FRAMES, predict_ref.NUMERIC
PRED, BEHIND, NFIN, BEHIND_R = predict_ref.PREDICTED, predict_ref.BEHIND, predict_ref.NOT_FINITE, predict_ref.BEHIND_RIGHT


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _part(r, i):
    """window i's outputs, every array of them"""
    a, b = r.offsets[i], r.offsets[i + 1]
    return ([r.pts_cam[a:b], r.flags[a:b], r.next_pose[i], np.asarray(r.n_predicted[i]), np.asarray(r.status[i])]
            + ([r.pts_cam_right[a:b]] if r.pts_cam_right is not None else []))


def _bitwise(x, y):
    for a, b in zip(x, y):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert a.tobytes() == b.tobytes()


def _state(ws):
    return [a.copy() for w in ws for a in w.state_arrays()]


def _check_parity(r, i, w, tag, mode="constant_velocity", given=None, want_status=OK):
    """window i of the report against the definition at w's state arrays: no landmark is left out; returns the largest error"""
    a, b = r.offsets[i], r.offsets[i + 1]
    right = r.pts_cam_right is not None
    ref = predict_ref.window_prediction(w, mode, given, right)
    assert ref.status == want_status and r.status[i] == want_status, (tag, ref.status, r.status[i])
    sel = ref.selected
    # the flag bits are decided clear of rounding, on the reference's values
    assert (np.abs(ref.pts_cam[sel, 2]) >= Z_CLEAR).all() and (not right or (np.abs(ref.pts_cam_right[sel, 2]) >= Z_CLEAR).all()), tag
    e = predict_ref.point_error(r.pts_cam[a:b], ref.pts_cam)
    er = predict_ref.point_error(r.pts_cam_right[a:b], ref.pts_cam_right) if right else 0.0
    ep = predict_ref.pose_error(r.next_pose[i], ref.next_pose)
    print("MEASURED %s %s: pts_cam %.1e, pts_cam_right %.1e, next_pose %.1e (tolerance %.0e); %d of %d predicted"
          % (tag, mode, e, er, ep, predict_ref.TOL, ref.n_predicted, w.L))
    np.testing.assert_array_equal(r.flags[a:b], ref.flags, err_msg=tag)
    assert r.n_predicted[i] == ref.n_predicted == int((r.flags[a:b] & PRED).sum()), tag
    assert max(e, er, ep) <= predict_ref.TOL, (tag, mode, e, er, ep)
    assert not r.pts_cam[a:b][~sel].any() and (not right or not r.pts_cam_right[a:b][~sel].any()), tag
    if want_status != OK:
        assert r.next_pose[i].tobytes() == w.pose[w.F - 1].tobytes(), tag
    return max(e, er, ep)


@pytest.mark.parametrize("name", list(SHAPES) + list(FIELD))
def test_parity_with_numpy(ctx, name):
    """the packing shapes (L9 padded lanes, L70 several start frames in a wave, L456 two chunks per start frame, F6 six frames) and the
    field windows (ragged tracks; f60_partial8: eight frames), at the initial state and after a 4-iteration solve, both modes, with and
    without the right camera; with L70 a copy of it with skew extrinsics"""
    from cerberus_amd import api
    w = (shape_window(name) if name in SHAPES else field_window(name)).twin()
    b = api.Batch(ctx, [w])
    worst = 0.0
    for state in ("initial", "solved"):
        if state == "solved":
            b.solve(api.default_solve_opts(True, 4))
            b.download()
        runs = [(b, w, "%s %s" % (name, state))]
        if name == "L70":
            sk = skew_extrinsics(w)
            runs.append((api.Batch(ctx, [sk]), sk, "L70 skew extrinsics %s" % state))
        for bb, ww, tag in runs:
            g = given_pose(ww)
            for mode, right in itertools.product(MODES, (False, True)):
                gi = g[None] if mode == "given" else None
                r = bb.predict_next_frame(mode, gi, right)
                assert (r.pts_cam_right is not None) == right and list(r.offsets) == [0, ww.L]
                worst = max(worst, _check_parity(r, 0, ww, tag + (" right" if right else ""), mode, g if mode == "given" else None))
    print("MEASURED %s: largest error %.1e (floor %.0e, tolerance %.0e)" % (name, worst, predict_ref.FLOOR, predict_ref.TOL))


def test_given_with_the_constant_velocity_pose_is_bitwise(ctx):
    """one code path after the pose: the given mode on the pose the constant-velocity mode returned gives its points and flags again"""
    from cerberus_amd import api
    ws = [shape_window("L70").twin(), field_window("f40").twin(), shape_window("F6").twin(), skew_extrinsics(shape_window("L9"))]
    b = api.Batch(ctx, ws)
    for state in ("initial", "solved"):
        if state == "solved":
            b.solve(api.default_solve_opts(True, 4))
        cv = b.predict_next_frame(right=True)
        gv = b.predict_next_frame("given", cv.next_pose, right=True)
        assert list(cv.status) == [OK] * 4 and cv.n_predicted.min() > 0
        for x, y in ((cv.pts_cam, gv.pts_cam), (cv.pts_cam_right, gv.pts_cam_right), (cv.flags, gv.flags), (cv.n_predicted, gv.n_predicted)):
            assert x.tobytes() == y.tobytes()
        assert np.abs(cv.next_pose - gv.next_pose).max() <= predict_ref.TOL


def test_behind_the_camera(ctx):
    """the next pose turned by pi about the body's vertical axis (the generator's body frame is the camera's, ric near the identity: the
    vertical axis is y): every predicted landmark is behind both cameras, the values still hold the tolerance"""
    from cerberus_amd import api
    ws = [shape_window("L70").twin(), field_window("f40").twin()]
    g = np.array([np.concatenate([w.pose[w.F - 1, :3], predict_ref.quat_mul(w.pose[w.F - 1, 3:7], [0.0, 1.0, 0.0, 0.0])]) for w in ws])
    r = api.Batch(ctx, ws).predict_next_frame("given", g, right=True)
    for i, w in enumerate(ws):
        _check_parity(r, i, w, "behind the camera %d" % i, "given", g[i])
        f = r.flags[r.offsets[i]:r.offsets[i + 1]]
        assert (f & PRED).any() and (f[(f & PRED) != 0] == PRED | BEHIND | BEHIND_R).all()


def test_unpredicted_landmarks(ctx):
    from cerberus_amd import api
    ws = [shape_window("L70").twin(), field_window("f40").twin()]
    neg = np.array([0, 3, 17, 64, 69])
    assert (predict_ref.selection(ws[0])[neg]).all()   # they end at the last frame: the depth alone takes them out
    ws[0].inv_depth[neg] = -1.0
    b = api.Batch(ctx, ws)
    r = b.predict_next_frame(right=True)
    out0 = (r.flags[:70] & PRED) == 0
    assert list(np.flatnonzero(out0)) == list(neg)
    assert list(np.flatnonzero(out0)) == list(np.flatnonzero(b.residuals().lm_flags[:70] & 2))   # the residual report's negative depths
    for i, w in enumerate(ws):
        _check_parity(r, i, w, "unpredicted %d" % i)
        a, e = r.offsets[i], r.offsets[i + 1]
        out = ~predict_ref.selection(w)
        assert out.any() and (~out).any()
        assert not r.pts_cam[a:e][out].any() and not r.pts_cam_right[a:e][out].any() and not r.flags[a:e][out].any()
        assert r.n_predicted[i] == (~out).sum()


def _frames(F):
    """the first F frames of the 70-landmark window"""
    from test_gpu_parity import _truncate
    w = shape_window("L70").twin()
    w.prior = w.prior.copy()   # (_truncate switches the prior off in place: not the cached window's)
    return _truncate(w, F)


def test_frame_counts(ctx):
    """two frames: TOO_FEW_FRAMES in the constant-velocity mode, a prediction in the given mode; three frames: the smallest window the
    constant-velocity mode predicts; alone and between 11-frame windows, bit for bit the same"""
    from cerberus_amd import api
    w2, w3, full = _frames(2), _frames(3), shape_window("L9")
    assert w2.L > 0 and w3.L > w2.L
    mixed = [full.twin(), w2.twin(), full.twin(), w3.twin()]
    g = np.array([given_pose(w) for w in mixed])
    for mode in MODES:
        rm = api.Batch(ctx, mixed).predict_next_frame(mode, g if mode == "given" else None, right=True)
        for w, pos in ((w2, 1), (w3, 3)):
            gi = g[pos] if mode == "given" else None
            ra = api.Batch(ctx, [w.twin()]).predict_next_frame(mode, gi[None] if mode == "given" else None, right=True)
            _bitwise(_part(rm, pos), _part(ra, 0))
            few = w.F == 2 and mode == "constant_velocity"
            _check_parity(rm, pos, w, "%d frames" % w.F, mode, gi, TOO_FEW if few else OK)
            assert (rm.n_predicted[pos] == 0 and not rm.flags[rm.offsets[pos]:rm.offsets[pos + 1]].any()) if few else rm.n_predicted[pos] > 0
        assert list(rm.status[[0, 2]]) == [OK, OK]


def test_non_finite_windows_fail_alone(ctx):
    """a NaN in a pose quaternion, or in a given pose: NUMERIC there, nothing predicted, frame k's pose reported; the neighbours are what
    they are alone"""
    from cerberus_amd import api
    good = [shape_window("L9"), shape_window("L70")]
    bad = shape_window("L70").twin()
    bad.pose[4, 4] = np.nan
    ws = [good[0].twin(), bad, good[1].twin()]
    g = np.array([given_pose(good[0]), given_pose(good[1]), given_pose(good[1])])
    for mode in MODES:
        gi = g if mode == "given" else None
        r = api.Batch(ctx, ws).predict_next_frame(mode, gi, right=True)
        assert list(r.status) == [OK, NUMERIC, OK] and r.n_predicted[1] == 0
        a, e = r.offsets[1], r.offsets[2]
        assert not r.pts_cam[a:e].any() and not r.pts_cam_right[a:e].any() and not r.flags[a:e].any()
        assert r.next_pose[1].tobytes() == bad.pose[10].tobytes()
        for pos, w in ((0, good[0]), (2, good[1])):
            alone = api.Batch(ctx, [w.twin()]).predict_next_frame(mode, g[pos][None] if mode == "given" else None, right=True)
            _bitwise(_part(r, pos), _part(alone, 0))
    g[2, 5] = np.nan
    r = api.Batch(ctx, [w.twin() for w in (good[0], good[1], good[1])]).predict_next_frame("given", g)
    assert list(r.status) == [OK, OK, NUMERIC] and r.n_predicted[2] == 0 and r.n_predicted[1] == 70
    assert not r.flags[r.offsets[2]:].any() and r.next_pose[2].tobytes() == good[1].pose[10].tobytes()
    # a NaN in the right camera's extrinsics matters only where the right camera is asked for
    nr = good[0].twin()
    nr.ex_pose[1, 0] = np.nan
    b = api.Batch(ctx, [nr])
    assert b.predict_next_frame().status[0] == OK and b.predict_next_frame(right=True).status[0] == NUMERIC


def test_window_without_landmarks(ctx, cfg, ocfg):
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    e0 = _no_landmarks(_window(cfg, ocfg, seed=62, L=10))
    r = api.Batch(ctx, [e0.twin()]).predict_next_frame(right=True)
    assert list(r.offsets) == [0, 0] and r.pts_cam.shape == (0, 3) and r.status[0] == OK and r.n_predicted[0] == 0
    _check_parity(r, 0, e0, "no landmarks")
    # the C entry point on such a batch: the pose and the records are reported, the caller's landmark arrays are untouched
    b = api.Batch(ctx, [e0.twin(), e0.twin()])
    p, f, pose, rec = np.full((3, 3), 7.0), np.full(3, 9, np.uint8), np.zeros((2, 7)), (T.WindowPredictRecord * 2)()
    rec[0].status = rec[1].status = 5
    dp = C.POINTER(C.c_double)
    assert api.lib().vilo_batch_predict_next_frame(ctx.h, b.handle, None, None, p.ctypes.data_as(dp), p.ctypes.data_as(dp), T.u8ptr(f),
                                                   pose.ctypes.data_as(dp), rec) == 0
    assert (p == 7.0).all() and (f == 9).all() and [rec[0].status, rec[1].status] == [OK, OK]
    assert pose[0].tobytes() == pose[1].tobytes() == r.next_pose[0].tobytes()
    assert api.lib().vilo_batch_predict_next_frame(ctx.h, b.handle, None, None, None, None, None, None, None) == 0
    # between windows that have landmarks
    w = shape_window("L9")
    alone = api.Batch(ctx, [w.twin()]).predict_next_frame(right=True)
    mixed = api.Batch(ctx, [e0.twin(), w.twin(), e0.twin()]).predict_next_frame(right=True)
    assert list(mixed.offsets) == [0, 0, 9, 9] and list(mixed.n_predicted) == [0, 9, 0] and list(mixed.status) == [OK] * 3
    _bitwise(_part(mixed, 1), _part(alone, 0))
    _bitwise(_part(mixed, 0), _part(r, 0))
    _bitwise(_part(mixed, 2), _part(r, 0))


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg):
    from cerberus_amd import api
    w = field_window("f40")
    other = _window(cfg, ocfg, seed=78, L=200)
    for mode in MODES:
        g = given_pose(w)
        go = given_pose(other)

        def run(ws):
            gi = np.array([g if x.L == w.L else go for x in ws]) if mode == "given" else None
            return api.Batch(ctx, ws).predict_next_frame(mode, gi, right=True)
        alone = _part(run([w.twin()]), 0)
        assert 0 < alone[3] < w.L
        eight = [other.twin() for _ in range(8)]
        eight[3] = w.twin()
        _bitwise(_part(run(eight), 3), alone)
        many = [other.twin() for _ in range(300)]
        for pos in (0, 150, 299):
            many[pos] = w.twin()
        r = run(many)
        for pos in (0, 150, 299):
            _bitwise(_part(r, pos), alone)


def _sequence(ctx, base, opts, report, samples):
    from cerberus_amd import api
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    if samples:
        b.set_samples()
    b.solve(opts)
    summ0 = b.download()
    before = _state(ws)
    if report:
        cv = b.predict_next_frame(right=True)
        b.predict_next_frame("given", cv.next_pose)
        summ1 = b.download()
        for x, y in zip(before, _state(ws)):
            assert x.tobytes() == y.tobytes()
        assert [bytes(s) for s in summ0] == [bytes(s) for s in summ1]
    b.solve(opts)
    replay = b.path()["replay"]
    summ = b.download()
    return _state(ws), [bytes(s) for s in summ], replay


@pytest.mark.parametrize("samples", [False, True])
def test_no_side_effects(ctx, cfg, ocfg, samples):
    """solve, predict in both modes, download: states and summaries bit for bit unchanged; the solve that follows (a replay of the
    captured graph where the batch has one) is bit for bit what it is without the calls"""
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s, L=60) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)
    st_a, su_a, rp_a = _sequence(ctx, base, opts, False, samples)
    st_b, su_b, rp_b = _sequence(ctx, base, opts, True, samples)
    for x, y in zip(st_a, st_b):
        assert x.tobytes() == y.tobytes()
    assert su_a == su_b and rp_a == rp_b
    if not samples:
        assert rp_b   # the second solve of a batch replays the graph the first one captured


def test_device_memory_is_returned(ctx, cfg, ocfg):
    from cerberus_amd import api
    ws = [_window(cfg, ocfg, seed=s, L=50) for s in (13, 14)]
    b = api.Batch(ctx, ws)
    bytes0 = b.device_bytes()   # nothing is kept with the batch: not even at the first call
    first = b.predict_next_frame(right=True)
    assert b.device_bytes() == bytes0
    for _ in range(5):
        r = b.predict_next_frame("given", first.next_pose, right=True)
        assert b.device_bytes() == bytes0
    r = b.predict_next_frame(right=True)
    for i in range(2):
        _bitwise(_part(r, i), _part(first, i))


def test_host_window_form_matches_batch(ctx):
    from cerberus_amd import api
    ws = [shape_window("L70").twin(), field_window("f40").twin(), shape_window("F6").twin()]
    ws[0].inv_depth[::5] = -1.0
    g = np.array([given_pose(w) for w in ws])
    for mode in MODES:
        gi = g if mode == "given" else None
        r = api.Batch(ctx, [w.twin() for w in ws]).predict_next_frame(mode, gi, right=True)
        tw = [w.twin() for w in ws]
        h = ctx.window_predict_next_frame(tw, mode, gi, right=True)
        for i in range(3):
            _bitwise(_part(h, i), _part(r, i))
            for x, y in zip(tw[i].state_arrays(), ws[i].state_arrays()):
                assert x.tobytes() == y.tobytes()   # the windows are left alone


def test_bad_arguments(ctx):
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    w = shape_window("L9").twin()
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_predict_next_frame
    dp = C.POINTER(C.c_double)
    p, pr, fl, pose, g = np.zeros((9, 3)), np.zeros((9, 3)), np.zeros(9, np.uint8), np.zeros((1, 7)), given_pose(w)[None].copy()
    rec = (T.WindowPredictRecord * 1)()
    pp, ppr, pf, ppose, pg = p.ctypes.data_as(dp), pr.ctypes.data_as(dp), T.u8ptr(fl), pose.ctypes.data_as(dp), g.ctypes.data_as(dp)

    def opts(**kw):
        o = T.PredictOpts()
        api.lib().vilo_default_predict_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    o = T.PredictOpts(7, 7)
    api.lib().vilo_default_predict_opts(C.byref(o))
    assert (o.mode, o.pad) == (0, 0)
    assert f(None, b.handle, opts(), None, pp, ppr, pf, ppose, rec) == -2
    assert f(ctx.h, None, opts(), None, pp, ppr, pf, ppose, rec) == -2
    assert f(ctx.h, b.handle, opts(), None, None, ppr, pf, ppose, rec) == -2       # NULL pts_cam with landmarks present
    for bad in (2, -1):
        assert f(ctx.h, b.handle, opts(mode=bad), pg, pp, ppr, pf, ppose, rec) == -2
    assert f(ctx.h, b.handle, opts(mode=1), None, pp, ppr, pf, ppose, rec) == -2   # GIVEN without next_pose_in
    h = api.lib().vilo_window_predict_next_frame
    ds, ss = w.desc(T)
    assert h(ctx.h, 0, C.byref(ds), C.byref(ss), opts(), None, pp, ppr, pf, ppose, rec) == -2
    assert h(ctx.h, 1, C.byref(ds), C.byref(ss), opts(mode=1), None, pp, ppr, pf, ppose, rec) == -2
    assert h(ctx.h, 1, C.byref(ds), C.byref(ss), opts(mode=3), pg, pp, ppr, pf, ppose, rec) == -2
    assert not p.any() and not pr.any() and not fl.any() and not pose.any() and rec[0].n_predicted == 0 and rec[0].status == 0
    # the batch is still usable; NULL options are the defaults, every output but pts_cam may be left out
    assert f(ctx.h, b.handle, None, None, pp, None, None, None, None) == 0
    r = b.predict_next_frame(right=True)
    assert p.tobytes() == r.pts_cam.tobytes() and r.n_predicted[0] == 9
    assert api.lib().vilo_last_predict_ms(ctx.h) > 0.0
    assert f(ctx.h, b.handle, opts(mode=1), pg, pp, ppr, pf, ppose, rec) == 0 and rec[0].status == OK and rec[0].n_predicted == 9
    assert h(ctx.h, 1, C.byref(ds), C.byref(ss), None, None, pp, ppr, pf, ppose, rec) == 0
    assert p.tobytes() == r.pts_cam.tobytes() and pr.tobytes() == r.pts_cam_right.tobytes() and fl.tobytes() == r.flags.tobytes()
    assert pose[0].tobytes() == r.next_pose[0].tobytes()
    _check_parity(r, 0, w, "after bad arguments")
