"""GPU (-m gpu): vilo_batch_landmark_covariance / vilo_window_landmark_covariance against the numpy definition (tests/lm_cov_ref.py: the
landmark rows of the full inverse of ref_gradient's dense problem at the state the device returns), bitwise agreement of frames / poses with
vilo_batch_covariance, freedom from side effects, independence of batch size, position and chunk, landmark order, per-window NaN, windows
without landmarks, the host-window form and bad arguments. Tolerances: lm_cov_ref.tolerances, ten times the FP64 floor
tests/test_landmark_covariance.py measures."""
import ctypes as C

import numpy as np
import pytest

import lm_cov_ref
from test_covariance_gpu import CASES, _solved, _window

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _window_slice(r, w):
    a, b = int(r.offsets[w]), int(r.offsets[w + 1])
    return r.inv_depth_var[a:b], r.points[a:b], r.point_cov[a:b]


def _assert_points_close(a, b, tag=""):
    """relative to each point's distance from the origin (a component near zero carries the rounding of the others)"""
    err = np.abs(a - b).max(axis=1) / np.linalg.norm(b, axis=1)
    assert err.max() <= lm_cov_ref.TOL_POINT, (tag, float(err.max()))


def _check_parity(r, w, ocfg, gauge, has_prior, tag, i=0):
    var, pts, pc = _window_slice(r, i)
    var_r, pts_r, pc_r = lm_cov_ref.landmark_covariance(ocfg, w, gauge=gauge)
    e = lm_cov_ref.errors(var, pc, var_r, pc_r)
    tv, tp = lm_cov_ref.tolerances(has_prior)
    assert e["var"] < tv and e["pcov"] < tp, (tag, gauge, e)
    _assert_points_close(pts, pts_r, tag)
    np.testing.assert_array_equal(pc, np.transpose(pc, (0, 2, 1)))
    assert np.all(var > 0) and np.all(np.linalg.eigvalsh(pc) > -1e-12 * np.abs(pc).max())


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_numpy(ctx, cfg, ocfg, case):
    w = _window(cfg, ocfg, seed=101 + len(case), **CASES[case])
    b = _solved(ctx, [w])
    has_prior = bool(w.prior.struct.valid)
    gauges = ["frame0", "none"] if case == "prior" else ["frame0"]
    for g in gauges:
        r = b.landmark_covariance(gauge=g)
        assert r.status[0] == 0 and r.offsets[-1] == w.L, (case, g, r.status)
        _check_parity(r, w, ocfg, g, has_prior, case)


def test_field_windows(ctx, cfg, ocfg):
    """The windows of tests/field_windows.py, each twice in one solved batch, against the numpy definition at test_parity_with_numpy's
    tolerances — the inverse-depth variance of a landmark with ONE two-residual factor among them; the two positions bitwise the same."""
    import field_windows as FW
    ws, names = FW.batch_of(FW.field_set(cfg, ocfg, FW.BATCH_NAMES), 2 * len(FW.BATCH_NAMES))
    b = _solved(ctx, ws, iters=FW.ITERS)
    r = b.landmark_covariance(gauge="frame0")
    for nm in FW.BATCH_NAMES:
        i = names.index(nm)
        w = ws[i]
        assert r.status[i] == 0, (nm, r.status)
        has_prior = bool(w.prior.struct.valid)
        _check_parity(r, w, ocfg, "frame0", has_prior, "field " + nm, i)
        one = int(np.flatnonzero(FW.factor_counts(w) == 1)[0])
        var = _window_slice(r, i)[0]
        var_r = lm_cov_ref.landmark_covariance(ocfg, w, gauge="frame0")[0]
        e_one = abs(var[one] - var_r[one]) / var_r[one]
        print("MEASURED landmark covariance of field window %s: one-factor landmark %d, variance %.3e, relative error %.1e" % (nm, one, var[one], e_one))
        assert e_one < lm_cov_ref.tolerances(has_prior)[0], (nm, e_one)
        for x, y in zip(_window_slice(r, names.index(nm, i + 1)), _window_slice(r, i)):
            np.testing.assert_array_equal(x, y)


def test_points_are_pub_point_cloud(ctx, cfg, ocfg):
    """points = R_s (R_c f / rho + t_c) + P_s at the downloaded state, to 1e-12 of the point's norm"""
    ws = [_window(cfg, ocfg, seed=s, L=90) for s in (41, 42)]
    b = _solved(ctx, ws)
    r = b.landmark_covariance()
    for i, w in enumerate(ws):
        _, pts, _ = _window_slice(r, i)
        _assert_points_close(pts, lm_cov_ref.world_points(w), i)


def test_frames_and_poses_match_state_covariance(ctx, cfg, ocfg):
    ws = [_window(cfg, ocfg, seed=s, L=60) for s in (51, 52)]
    b = _solved(ctx, ws)
    for g in ("frame0", "none"):
        fr, po, st = b.covariance(gauge=g, poses=True)
        r = b.landmark_covariance(gauge=g, frames=True, poses=True)
        np.testing.assert_array_equal(r.frames, fr)
        np.testing.assert_array_equal(r.poses, po)
        np.testing.assert_array_equal(r.status, st)
        fr0, _, _ = b.covariance(gauge=g)
        r0 = b.landmark_covariance(gauge=g, frames=True)
        assert r0.poses is None
        np.testing.assert_array_equal(r0.frames, fr0)
        r1 = b.landmark_covariance(gauge=g)
        assert r1.frames is None and r1.poses is None
        for x, y in ((r.inv_depth_var, r1.inv_depth_var), (r.points, r1.points), (r.point_cov, r1.point_cov)):
            np.testing.assert_array_equal(x, y)


def test_no_side_effects(ctx, cfg, ocfg):
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)
    ws_a = [w.twin() for w in base]
    a = api.Batch(ctx, ws_a)
    a.solve(opts)
    a.download()
    a.solve(opts)
    summ_a = a.download()
    ws_b = [w.twin() for w in base]
    b = api.Batch(ctx, ws_b)
    b.solve(opts)
    summ0 = b.download()
    before = [s.copy() for w in ws_b for s in w.state_arrays()]
    b.landmark_covariance(frames=True, poses=True)
    b.landmark_covariance()
    summ1 = b.download()
    after = [s.copy() for w in ws_b for s in w.state_arrays()]
    for x, y in zip(before, after):
        np.testing.assert_array_equal(x, y)
    for s0, s1 in zip(summ0, summ1):
        assert bytes(s0) == bytes(s1)
    b.solve(opts)
    summ_b = b.download()
    for wa, wb in zip(ws_a, ws_b):
        for x, y in zip(wa.state_arrays(), wb.state_arrays()):
            np.testing.assert_array_equal(x, y)
    for sa, sb in zip(summ_a, summ_b):
        assert bytes(sa) == bytes(sb)


def test_independent_of_batch_size_position_and_chunk(ctx, cfg, ocfg):
    """bitwise the same landmark outputs wherever the window sits, a window of the second 4096-window chunk included"""
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=77, L=80)
    other = _window(cfg, ocfg, seed=78, L=40)
    b1 = _solved(ctx, [w.twin()], iters=3)
    ref = b1.landmark_covariance()
    assert ref.status[0] == 0
    w.set_state([a.copy() for a in b1.windows[0].state_arrays()])
    for W, positions in ((128, (0, 65, 127)), (4097, (1, 4096))):
        ws = [other.twin() for _ in range(W)]
        for p in positions:
            ws[p] = w.twin()
        bb = api.Batch(ctx, ws)   # windows at their (given) states: the covariance is evaluated there
        r = bb.landmark_covariance()
        for p in positions:
            assert r.status[p] == 0
            for x, y in zip(_window_slice(r, p), _window_slice(ref, 0)):
                np.testing.assert_array_equal(x, y, err_msg="W=%d pos=%d" % (W, p))
        bb.close()


def _permuted(w, perm):
    """a twin of w whose landmarks are listed in the order perm (new landmark i = old landmark perm[i])"""
    t = w.twin()
    obs, st, off = [], [], [0]
    for l in perm:
        o0, o1 = w.lm_obs_offset[l], w.lm_obs_offset[l + 1]
        obs.append(w.obs[o0:o1]); st.append(w.obs_is_stereo[o0:o1]); off.append(off[-1] + (o1 - o0))
    t.obs = np.ascontiguousarray(np.concatenate(obs)); t.obs_is_stereo = np.ascontiguousarray(np.concatenate(st))
    t.lm_obs_offset = np.array(off, np.int32)
    t.lm_start_frame = np.ascontiguousarray(w.lm_start_frame[perm])
    t.inv_depth = np.ascontiguousarray(w.inv_depth[perm])
    return t


def test_landmark_order_follows_the_descriptor(ctx, cfg, ocfg):
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=88, L=100)
    b = _solved(ctx, [w])
    r = b.landmark_covariance()
    perm = np.random.default_rng(3).permutation(w.L)
    r2 = api.Batch(ctx, [_permuted(w, perm)]).landmark_covariance()
    assert r2.status[0] == 0
    e = lm_cov_ref.errors(r2.inv_depth_var, r2.point_cov, r.inv_depth_var[perm], r.point_cov[perm])
    tv, tp = lm_cov_ref.tolerances(True)
    assert e["var"] < tv and e["pcov"] < tp, e
    _assert_points_close(r2.points, r.points[perm])


def test_rank_deficiency_is_per_window(ctx, cfg, ocfg):
    wp = _window(cfg, ocfg, seed=5, L=50)
    wn = _window(cfg, ocfg, seed=6, L=50, prior=False)
    b = _solved(ctx, [wp.twin(), wn.twin(), wp.twin()])
    r = b.landmark_covariance(gauge="none")
    assert list(r.status) == [0, 1, 0]
    for x in _window_slice(r, 1):
        assert np.isnan(x).all()
    alone = _solved(ctx, [wp.twin()]).landmark_covariance(gauge="none")
    assert alone.status[0] == 0
    for p in (0, 2):
        for x, y in zip(_window_slice(r, p), _window_slice(alone, 0)):
            assert np.isfinite(x).all()
            np.testing.assert_array_equal(x, y)


def _no_landmarks(w):
    w.L, w.n_obs = 0, 0
    w.lm_start_frame = np.zeros(0, np.int32); w.lm_obs_offset = np.zeros(1, np.int32)
    w.obs = np.zeros((0, 11)); w.obs_is_stereo = np.zeros(0, np.uint8); w.inv_depth = np.zeros(0)
    return w


def test_windows_without_landmarks(ctx, cfg, ocfg):
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=61, L=70)
    e0 = _no_landmarks(_window(cfg, ocfg, seed=62, L=10))
    b = _solved(ctx, [w])
    ref = b.landmark_covariance()
    mixed = api.Batch(ctx, [e0.twin(), w.twin(), e0.twin()])
    r = mixed.landmark_covariance()
    assert list(r.offsets) == [0, 0, w.L, w.L] and r.inv_depth_var.shape == (w.L,)
    for x, y in zip(_window_slice(r, 1), _window_slice(ref, 0)):
        np.testing.assert_array_equal(x, y)
    only = api.Batch(ctx, [e0.twin()]).landmark_covariance(frames=True)
    assert only.inv_depth_var.shape == (0,) and only.points.shape == (0, 3) and only.frames.shape == (1, 11, 19, 19)
    fr, _, st = api.Batch(ctx, [e0.twin()]).covariance()
    assert only.status[0] == st[0]
    np.testing.assert_array_equal(only.frames, fr)


def test_host_window_form_matches_batch(ctx, cfg, ocfg):
    ws = [_window(cfg, ocfg, seed=s, L=70) for s in (21, 22, 23)]
    b = _solved(ctx, ws)
    r = b.landmark_covariance(poses=True)
    h = ctx.window_landmark_covariance(ws, poses=True)
    assert list(r.status) == list(h.status) == [0, 0, 0]
    assert list(r.offsets) == list(h.offsets)
    for x, y in ((h.inv_depth_var, r.inv_depth_var), (h.points, r.points), (h.point_cov, r.point_cov), (h.poses, r.poses)):
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-14 * np.abs(y).max())


def test_bad_arguments(ctx, cfg, ocfg):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    b = _solved(ctx, [_window(cfg, ocfg, seed=3, L=40)], iters=2)
    with pytest.raises(ValueError):
        b.landmark_covariance(gauge="world")
    L = 40
    var, pts, pc, st = np.zeros(L), np.zeros((L, 3)), np.zeros((L, 3, 3)), np.zeros(1, np.int32)
    f = api.lib().vilo_batch_landmark_covariance
    o = api.default_cov_opts()
    o.gauge = 7
    assert f(ctx.h, b.handle, C.byref(o), None, None, T.dptr(var), T.dptr(pts), T.dptr(pc), T.iptr(st)) == -2
    o = api.default_cov_opts()
    o.min_reciprocal_condition = -1.0
    assert f(ctx.h, b.handle, C.byref(o), None, None, T.dptr(var), T.dptr(pts), T.dptr(pc), T.iptr(st)) == -2
    o = api.default_cov_opts()
    assert f(ctx.h, b.handle, C.byref(o), None, None, None, T.dptr(pts), T.dptr(pc), T.iptr(st)) == -2
    assert f(ctx.h, b.handle, C.byref(o), None, None, T.dptr(var), T.dptr(pts), T.dptr(pc), None) == -2
    assert f(None, b.handle, C.byref(o), None, None, T.dptr(var), T.dptr(pts), T.dptr(pc), T.iptr(st)) == -2
    # opts->want_poses is ignored: no poses buffer is written or required
    o.want_poses = 1
    assert f(ctx.h, b.handle, C.byref(o), None, None, T.dptr(var), T.dptr(pts), T.dptr(pc), T.iptr(st)) == 0
    assert st[0] == 0 and np.isfinite(var).all()
