"""GPU (-m gpu): vilo_batch_frame_pose_pnp / vilo_window_frame_pose_pnp against the numpy definition (tests/pnp_ref.py) at the state the
device returns: parity on the packing shapes, too few points and frames out of range, independence of batch size and position, freedom
from side effects, the write-back and what follows it (triangulation, solve, graph replay), the host form, the call's device memory, bad
arguments, a single step. Tolerances: ten times the FP64 floor tests/test_pnp.py measures (pnp_ref.TOL_POS / TOL_ROT)."""
import ctypes as C

import numpy as np
import pytest

import pnp_ref
import tri_ref
from test_covariance_gpu import _window
from test_landmark_covariance_gpu import _no_landmarks
from test_triangulate import SHAPES, shape_window, third_mono

pytestmark = pytest.mark.gpu

OK, FEW, NOCONV, NUMERIC, NOFRAME = pnp_ref.OK, pnp_ref.NOT_ENOUGH_POINTS, pnp_ref.NO_CONVERGENCE, pnp_ref.NUMERIC, pnp_ref.NO_FRAME


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _row(r, i):
    return [np.ascontiguousarray(r.pose[i])] + [np.asarray(x[i]) for x in r[1:]]


def _bitwise(x, y):
    for a, b in zip(x, y):
        assert a.shape == b.shape and a.dtype == b.dtype
        assert a.tobytes() == b.tobytes()


def _state(ws):
    return [a.copy() for w in ws for a in w.state_arrays()]


def _check_parity(r, i, w, tag, frame, guess, max_iterations=20):
    """window i of the report against the definition at w's state arrays"""
    ref = pnp_ref.frame_pose(w, frame, guess)
    assert ref.status == OK, tag
    assert r.status[i] == OK and r.n_points[i] == ref.n_points and 1 <= r.iterations[i] <= max_iterations, (tag, r.status[i], r.n_points[i], r.iterations[i])
    ep, er = pnp_ref.pose_errors(r.pose[i], ref.R, ref.P)
    ec = abs(r.final_cost[i] - ref.final_cost) / ref.final_cost
    print("MEASURED %s: position %.1e (tolerance %.0e), rotation %.1e (tolerance %.0e), cost %.1e, steps %d (reference %d)"
          % (tag, ep, pnp_ref.TOL_POS, er, pnp_ref.TOL_ROT, ec, r.iterations[i], ref.iterations))
    assert ep <= pnp_ref.TOL_POS and er <= pnp_ref.TOL_ROT, (tag, ep, er)
    assert ec <= pnp_ref.TOL_COST, (tag, ec)
    assert abs(r.initial_cost[i] - ref.initial_cost) <= pnp_ref.TOL_COST * ref.initial_cost, tag
    assert r.pose[i, 6] >= 0.0 and abs(np.linalg.norm(r.pose[i, 3:7]) - 1.0) <= 4e-16
    return ref


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_parity_with_numpy(ctx, shape):
    from cerberus_amd import api
    ws = [shape_window(shape).twin(), third_mono(shape_window(shape))]
    b = api.Batch(ctx, ws)
    for state in ("initial", "solved"):
        if state == "solved":
            b.solve(api.default_solve_opts(True, 4))
            b.download()
        for frame in (-1, 2, ws[0].F // 2):
            for guess in ("previous", "current"):
                r = b.frame_pose_pnp(frame, guess, step_tolerance=pnp_ref.PARITY_STEP_TOLERANCE)
                for i, name in enumerate(("stereo", "third mono")):
                    _check_parity(r, i, ws[i], "%s %s %s frame %d %s" % (shape, name, state, frame, guess), frame, guess)
                    if guess == "current" and state == "solved":
                        assert r.final_cost[i] <= r.initial_cost[i]


def _few_depths(w, keep=3):
    """a copy of w with all but `keep` of the last frame's usable inverse depths set to -1"""
    t = w.twin()
    ids = pnp_ref.points(t, t.F - 1)[2]
    t.inv_depth[ids[keep:]] = -1.0
    assert len(pnp_ref.points(t, t.F - 1)[2]) == keep
    return t


def test_too_few_points_and_no_frame(ctx):
    from cerberus_amd import api
    # L9 has two points on frame 1; the thinned L70 three on its last frame
    for w, frame, n in ((shape_window("L9"), 1, 2), (_few_depths(shape_window("L70")), 10, 3)):
        ws = [w.twin()]
        st0 = _state(ws)
        b = api.Batch(ctx, ws)
        for write in (False, True):
            r = b.frame_pose_pnp(frame, write=write)
            assert (r.status[0], r.n_points[0], r.iterations[0]) == (FEW, n, 0)
            assert r.pose[0].tobytes() == w.pose[frame].tobytes()
        b.download()
        for x, y in zip(_state(ws), st0):
            assert x.tobytes() == y.tobytes()   # write = True on a failed window: the batch's state is bitwise unchanged
    # a frame beyond a six-frame window inside a mixed batch: NO_FRAME for that window only, which write = True leaves alone
    ws = [shape_window("L70").twin(), shape_window("F6").twin(), shape_window("L9").twin()]
    st0 = _state(ws)
    b = api.Batch(ctx, ws)
    for frame in (8, 6):
        r = b.frame_pose_pnp(frame, write=True)
        assert list(r.status) == [OK, NOFRAME, OK] and r.n_points[1] == 0 and r.iterations[1] == 0
        assert r.pose[1].tobytes() == np.array([0, 0, 0, 0, 0, 0, 1.0]).tobytes()   # row `frame` of the padded state
    b.download()
    st1 = _state(ws)
    for x, y in zip(st1[6:12], st0[6:12]):
        assert x.tobytes() == y.tobytes()
    assert st1[0][8].tobytes() != st0[0][8].tobytes()   # (the windows beside it were written)
    assert b.frame_pose_pnp(5).status[1] == OK


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg):
    from cerberus_amd import api
    w = third_mono(shape_window("L456"))
    others = [_window(cfg, ocfg, seed=78, L=200), shape_window("F6"), shape_window("L9"), shape_window("L70")]
    kw = dict(frame=7, guess="previous")
    alone = _row(api.Batch(ctx, [w.twin()]).frame_pose_pnp(**kw), 0)
    assert alone[5] == OK
    eight = [others[i % 4].twin() for i in range(8)]
    eight[3] = w.twin()
    _bitwise(_row(api.Batch(ctx, eight).frame_pose_pnp(**kw), 3), alone)
    many = [others[i % 4].twin() for i in range(300)]
    for pos in (0, 150, 299):
        many[pos] = w.twin()
    r = api.Batch(ctx, many).frame_pose_pnp(**kw)
    for pos in (0, 150, 299):
        _bitwise(_row(r, pos), alone)


def _sequence(ctx, base, opts, report):
    from cerberus_amd import api
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    b.solve(opts)
    b.download()
    before = _state(ws)
    res = None
    if report:
        b.frame_pose_pnp()
        b.frame_pose_pnp(2, "current")
        b.download()
        for x, y in zip(before, _state(ws)):
            assert x.tobytes() == y.tobytes()
    rr = b.residuals()
    res = [np.asarray(x).tobytes() for x in rr if x is not None]
    b.solve(opts)
    summ = b.download()
    return _state(ws), [bytes(s) for s in summ], res


def test_no_side_effects(ctx, cfg, ocfg):
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)
    st_a, su_a, re_a = _sequence(ctx, base, opts, False)
    st_b, su_b, re_b = _sequence(ctx, base, opts, True)
    for x, y in zip(st_a, st_b):
        assert x.tobytes() == y.tobytes()
    assert su_a == su_b and re_a == re_b


@pytest.mark.parametrize("replay", [False, True])
def test_write_back(ctx, replay):
    from cerberus_amd import api
    opts = api.default_solve_opts(True, 4)
    base = [third_mono(shape_window("L70")), shape_window("F6").twin()]
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    if replay:
        b.solve(opts)   # solve once before the write: the solve after it replays the captured graph
        b.reset()
    b.download()
    before = _state(ws)
    k = 4
    r = b.frame_pose_pnp(k, write=True)
    assert list(r.status) == [OK, OK]
    b.download()
    after = _state(ws)
    for i, w in enumerate(ws):
        for j in range(6):
            x, y = after[6 * i + j], before[6 * i + j]
            if j == 0:   # pose: exactly row k changed, to the reported pose
                assert x[k].tobytes() == r.pose[i].tobytes() and x[k].tobytes() != y[k].tobytes()
                x = np.delete(x, k, 0); y = np.delete(y, k, 0)
            assert x.tobytes() == y.tobytes(), (i, j)
    # triangulation after it starts from the written pose
    t = b.triangulate("all", stereo=False)
    for i, w in enumerate(ws):
        ref = tri_ref.window_triangulation(w, "all", stereo=False)
        es, et = tri_ref.branch_errors(t.depth[t.offsets[i]:t.offsets[i + 1]], ref)
        assert es <= tri_ref.TOL_STEREO and et <= tri_ref.TOL_TWO_FRAME, (i, es, et)
    # so does the solve: a fresh batch created at that state gives the same, to the solver forms' own tolerance
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


def test_host_window_form_matches_batch(ctx):
    from cerberus_amd import api
    ws = [third_mono(shape_window("L70")), shape_window("L9").twin(), shape_window("F6").twin()]
    for frame in (1, 5):
        r = api.Batch(ctx, [w.twin() for w in ws]).frame_pose_pnp(frame)
        tw = [w.twin() for w in ws]
        h = ctx.window_frame_pose_pnp(tw, frame)
        for i in range(3):
            _bitwise(_row(h, i), _row(r, i))
            for x, y in zip(tw[i].state_arrays(), ws[i].state_arrays()):
                assert x.tobytes() == y.tobytes()   # write = 0: the windows are left alone
        tw = [w.twin() for w in ws]
        h = ctx.window_frame_pose_pnp(tw, frame, write=True)
        for i in range(3):
            _bitwise(_row(h, i), _row(r, i))
            want = ws[i].pose.copy()
            if h.status[i] == OK:
                want[frame] = h.pose[i]
            assert tw[i].pose.tobytes() == want.tobytes()
            for x, y in zip(tw[i].state_arrays()[1:], ws[i].state_arrays()[1:]):
                assert x.tobytes() == y.tobytes()
    assert h.status[1] == OK and r.status[0] == OK


def test_device_memory_is_returned(ctx, cfg, ocfg):
    from cerberus_amd import api
    b = api.Batch(ctx, [_window(cfg, ocfg, seed=s, L=50) for s in (13, 14)])
    bytes0 = b.device_bytes()
    first = b.frame_pose_pnp()
    assert b.device_bytes() == bytes0
    for _ in range(20):
        r = b.frame_pose_pnp()
        assert b.device_bytes() == bytes0
    for i in range(2):
        _bitwise(_row(r, i), _row(first, i))


def test_window_without_landmarks(ctx, cfg, ocfg):
    from cerberus_amd import api
    e0 = _no_landmarks(_window(cfg, ocfg, seed=62, L=10))
    r = api.Batch(ctx, [e0.twin()]).frame_pose_pnp()
    assert list(r.status) == [FEW] and list(r.n_points) == [0]
    assert r.pose[0].tobytes() == e0.pose[e0.F - 1].tobytes()
    w = shape_window("L9")
    alone = api.Batch(ctx, [w.twin()]).frame_pose_pnp()
    mixed = api.Batch(ctx, [e0.twin(), w.twin(), e0.twin()]).frame_pose_pnp()
    assert list(mixed.status) == [FEW, OK, FEW]
    _bitwise(_row(mixed, 1), _row(alone, 0))


def test_bad_arguments(ctx):
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    w = shape_window("L9").twin()
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_frame_pose_pnp
    pose, rec = np.zeros(7), (T.WindowPnpRecord * 1)()
    pp = pose.ctypes.data_as(T.c_double_p)

    def opts(**kw):
        o = T.PnpOpts()
        api.lib().vilo_default_pnp_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    assert f(None, b.handle, opts(), pp, rec) == -2
    assert f(ctx.h, None, opts(), pp, rec) == -2
    assert f(ctx.h, b.handle, opts(), None, rec) == -2          # NULL pose with windows present
    for bad in (2, -1):
        assert f(ctx.h, b.handle, opts(guess=bad), pp, rec) == -2
    for bad in (-2, 0, 11):
        assert f(ctx.h, b.handle, opts(frame=bad), pp, rec) == -2
    for bad in (0, -3, 65):
        assert f(ctx.h, b.handle, opts(max_iterations=bad), pp, rec) == -2
    for bad in (-1e-9, float("nan"), float("inf")):
        assert f(ctx.h, b.handle, opts(step_tolerance=bad), pp, rec) == -2
    g = api.lib().vilo_window_frame_pose_pnp
    ds, ss = w.desc(T)
    assert g(ctx.h, 0, C.byref(ds), C.byref(ss), opts(), pp, rec) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(frame=0), pp, rec) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(), None, rec) == -2
    assert not pose.any() and rec[0].status == 0 and rec[0].n_points == 0
    # the batch is still usable; NULL options are the defaults, the records may be left out
    assert f(ctx.h, b.handle, None, pp, None) == 0
    r = b.frame_pose_pnp()
    assert pose.tobytes() == r.pose[0].tobytes() and r.status[0] == OK
    assert api.lib().vilo_last_pnp_ms(ctx.h) > 0.0
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(frame=10), pp, rec) == 0 and rec[0].status == OK
    assert pose.tobytes() == r.pose[0].tobytes()


def test_one_iteration(ctx):
    from cerberus_amd import api
    ws = [third_mono(shape_window("L70")), shape_window("L456").twin()]
    r = api.Batch(ctx, ws).frame_pose_pnp(max_iterations=1)
    for i, w in enumerate(ws):
        ref = pnp_ref.frame_pose(w, -1, "previous", max_iterations=1, step_tolerance=1e-12)
        assert ref.status == NOCONV and r.status[i] == NOCONV and r.iterations[i] == 1 and r.n_points[i] == ref.n_points
        ep, er = pnp_ref.pose_errors(r.pose[i], ref.R, ref.P)
        print("MEASURED one step %d: position %.1e rotation %.1e" % (i, ep, er))
        assert ep <= pnp_ref.TOL_POS and er <= pnp_ref.TOL_ROT, (i, ep, er)
        assert abs(r.final_cost[i] - ref.final_cost) <= pnp_ref.TOL_COST * ref.final_cost
        assert r.final_cost[i] < r.initial_cost[i]
