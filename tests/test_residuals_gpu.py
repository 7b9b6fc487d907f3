"""GPU (-m gpu): vilo_batch_residuals / vilo_window_residuals against the numpy definition (tests/resid_ref.py) at the state the device
returns, against the solver's own costs, the reference's outlier / failure sets, freedom from side effects, independence of batch size and
position, edge windows, the host form and bad arguments."""
import ctypes as C

import numpy as np
import pytest

import resid_ref
from test_covariance_gpu import CASES, _solved, _window
from test_landmark_covariance_gpu import _no_landmarks

pytestmark = pytest.mark.gpu

SCALARS = ("cost", "prior_cost", "visual_cost", "visual_cost_plain")
COUNTS = ("n_visual_blocks", "n_huber_active", "n_outliers", "n_negative_depth", "status")


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _obs_offsets(windows):
    return np.concatenate([[0], np.cumsum([w.n_obs if w.L > 0 else 0 for w in windows])]).astype(np.int64)


def _window_part(r, i, obs_off):
    """window i's outputs, every array of them"""
    a, b = r.offsets[i], r.offsets[i + 1]
    out = [np.array([getattr(r, f)[i] for f in SCALARS]), r.imu_cost[i], np.array([getattr(r, f)[i] for f in COUNTS]),
           r.lm_cost[a:b], r.lm_reproj_px[a:b], r.lm_flags[a:b]]
    if r.obs_residuals is not None:
        out.append(r.obs_residuals[obs_off[i]:obs_off[i + 1]])
    if r.imu_residuals is not None:
        out.append(r.imu_residuals[i])
    return out


def _bitwise(x, y):
    for a, b in zip(x, y):
        assert a.shape == b.shape
        assert a.tobytes() == b.tobytes()


def _rel_le(a, b, tol):
    a, b = np.asarray(a, float), np.asarray(b, float)
    assert (np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))).all(), np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)))


def _check_parity(r, i, ref, obs_off):
    for f in SCALARS:
        _rel_le(getattr(r, f)[i], ref[f], 1e-12)
    _rel_le(r.imu_cost[i], ref["imu_cost"], 1e-12)
    for f in COUNTS:
        assert getattr(r, f)[i] == ref[f], f
    a, b = r.offsets[i], r.offsets[i + 1]
    _rel_le(r.lm_cost[a:b], ref["lm_cost"], 1e-12)
    np.testing.assert_allclose(r.lm_reproj_px[a:b], ref["lm_reproj_px"], rtol=1e-12, atol=0)
    np.testing.assert_array_equal(r.lm_flags[a:b], ref["lm_flags"])
    if r.obs_residuals is not None:
        ob = r.obs_residuals[obs_off[i]:obs_off[i + 1]]
        np.testing.assert_array_equal(np.isnan(ob), np.isnan(ref["obs_residuals"]))
        m = ~np.isnan(ob)
        assert (np.abs(ob[m] - ref["obs_residuals"][m]) <= 1e-12).all(), np.abs(ob[m] - ref["obs_residuals"][m]).max()
    if r.imu_residuals is not None:
        _rel_le(r.imu_residuals[i], ref["imu_residuals"], 1e-11)


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_numpy(ctx, cfg, ocfg, case):
    w = _window(cfg, ocfg, seed=301 + len(case), **CASES[case])
    b = _solved(ctx, [w])
    r = b.residuals(observations=True, imu=True)
    _check_parity(r, 0, resid_ref.window_residuals(ocfg, w), _obs_offsets([w]))
    if not w.use_leg:
        assert not r.imu_residuals[0, :, 15:].any()
    assert not r.imu_residuals[0, w.F - 1:].any() and not r.imu_cost[0, w.F - 1:].any()


def test_agrees_with_the_solver(ctx, cfg, ocfg):
    from cerberus_amd import api
    ws = [_window(cfg, ocfg, seed=s) for s in (31, 32)] + [_window(cfg, ocfg, seed=33, prior=False)]
    b = api.Batch(ctx, ws)
    r0 = b.residuals()
    b.solve(api.default_solve_opts(True, 6))
    summ = b.download()
    r1 = b.residuals()
    for i, s in enumerate(summ):
        assert abs(r0.cost[i] - s.initial_cost) <= 1e-12 * abs(s.initial_cost)
        assert abs(r1.cost[i] - s.final_cost) <= 1e-12 * abs(s.final_cost)
    for r in (r0, r1):
        for i in range(len(ws)):
            total = r.prior_cost[i] + r.imu_cost[i].sum() + r.visual_cost[i]
            assert abs(r.cost[i] - total) <= 1e-14 * abs(r.cost[i])
            lm = r.lm_cost[r.offsets[i]:r.offsets[i + 1]].sum()
            assert abs(r.visual_cost[i] - lm) <= 1e-14 * abs(r.visual_cost[i])
            assert r.visual_cost_plain[i] >= r.visual_cost[i]


def test_outliers_and_failures(ctx, cfg, ocfg):
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=4141, L=120)
    chosen = [3, 17, 40, 77, 101]
    resid_ref.shift_observations(w, chosen, 10.0, cfg.focal_length)
    b = _solved(ctx, [w])
    r = b.residuals()
    ref = resid_ref.window_residuals(ocfg, w)
    np.testing.assert_array_equal(r.lm_flags & 1, ref["lm_flags"] & 1)
    assert all(r.lm_flags[chosen] & 1)
    assert r.n_outliers[0] == int((ref["lm_flags"] & 1).sum())
    # a negative inverse depth in the initial state: setDepth's failure
    v = _window(cfg, ocfg, seed=4142, L=60)
    v.inv_depth[9] = -v.inv_depth[9]
    r = api.Batch(ctx, [v]).residuals()
    assert np.flatnonzero(r.lm_flags & 2).tolist() == [9] and r.n_negative_depth[0] == 1


def _sequence(ctx, base, opts, report, samples):
    from cerberus_amd import api
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    if samples:
        b.set_samples()
    b.solve(opts)
    summ0 = b.download()
    before = [s.copy() for w in ws for s in w.state_arrays()]
    if report:
        b.residuals(observations=True, imu=True)
        summ1 = b.download()
        for x, y in zip(before, [s.copy() for w in ws for s in w.state_arrays()]):
            np.testing.assert_array_equal(x, y)
        for s0, s1 in zip(summ0, summ1):
            assert bytes(s0) == bytes(s1)
    b.solve(opts)
    summ = b.download()
    return [s.copy() for w in ws for s in w.state_arrays()], [bytes(s) for s in summ]


@pytest.mark.parametrize("samples", [False, True])
def test_no_side_effects(ctx, cfg, ocfg, samples):
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)
    st_a, su_a = _sequence(ctx, base, opts, False, samples)
    st_b, su_b = _sequence(ctx, base, opts, True, samples)
    for x, y in zip(st_a, st_b):
        np.testing.assert_array_equal(x, y)
    assert su_a == su_b


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg):
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=77, L=80)
    other = _window(cfg, ocfg, seed=78, L=80)
    kw = dict(observations=True, imu=True)
    b1 = api.Batch(ctx, [w.twin()])
    alone, again = b1.residuals(**kw), b1.residuals(**kw)
    _bitwise(_window_part(alone, 0, _obs_offsets([w])), _window_part(again, 0, _obs_offsets([w])))
    three = [other.twin(), w.twin(), other.twin()]
    mid = api.Batch(ctx, three).residuals(**kw)
    _bitwise(_window_part(mid, 1, _obs_offsets(three)), _window_part(alone, 0, _obs_offsets([w])))
    many = [w.twin() for _ in range(1100)]
    big = api.Batch(ctx, many).residuals(**kw)
    oo = _obs_offsets(many)
    for i in (0, 549, 1099):
        _bitwise(_window_part(big, i, oo), _window_part(alone, 0, _obs_offsets([w])))
    # the same through the host form at the states a solve left
    s = _solved(ctx, [w.twin(), other.twin()])
    solved = s.windows
    h1 = ctx.window_residuals([solved[0]], **kw)
    h3 = ctx.window_residuals([solved[1], solved[0], solved[1]], **kw)
    _bitwise(_window_part(h3, 1, _obs_offsets([solved[1], solved[0], solved[1]])), _window_part(h1, 0, _obs_offsets([solved[0]])))


def test_edge_windows(ctx, cfg, ocfg):
    from cerberus_amd import api
    kw = dict(observations=True, imu=True)
    e0 = _no_landmarks(_window(cfg, ocfg, seed=62, L=10))
    nop = _window(cfg, ocfg, seed=63, L=40, prior=False)
    f6 = _window(cfg, ocfg, seed=64, L=40, F=6, prior=False, leg_bias_const=1)
    bad = _window(cfg, ocfg, seed=65, L=40)
    bad.preint = bad.preint.copy()
    bad.preint[2][33 + 961] = -1.0   # covariance (0, 0) of interval 2: not positive definite, no sqrt_info
    ws = [e0, nop, bad, f6]
    r = api.Batch(ctx, [w.twin() for w in ws]).residuals(**kw)
    oo = _obs_offsets(ws)
    assert list(r.offsets) == [0, 0, 40, 80, 80 + f6.L] and oo[1] == 0
    assert r.visual_cost[0] == 0.0 and r.n_visual_blocks[0] == 0 and r.status[0] == 0
    _check_parity(r, 0, resid_ref.window_residuals(ocfg, e0), oo)
    assert r.prior_cost[1] == 0.0
    _check_parity(r, 1, resid_ref.window_residuals(ocfg, nop), oo)
    _check_parity(r, 3, resid_ref.window_residuals(ocfg, f6), oo)
    assert not r.imu_cost[3, 5:].any() and not r.imu_residuals[3, 5:].any()
    assert r.status[2] == 2 and np.isnan(r.cost[2]) and np.isnan(r.imu_cost[2, 2]) and np.isnan(r.imu_residuals[2, 2]).all()
    assert np.isfinite(np.delete(r.imu_cost[2], 2)).all() and np.isfinite(r.visual_cost[2])
    # the neighbours are what they are alone
    for i, w in ((0, e0), (1, nop), (3, f6)):
        alone = api.Batch(ctx, [w.twin()]).residuals(**kw)
        _bitwise(_window_part(r, i, oo), _window_part(alone, 0, _obs_offsets([w])))
    # USE_LEG = 0 (a batch of its own: one IMU factor kind per batch)
    imu = _window(cfg, ocfg, seed=66, L=40, use_leg=0, leg_bias_const=1)
    r = api.Batch(ctx, [imu.twin()]).residuals(**kw)
    _check_parity(r, 0, resid_ref.window_residuals(ocfg, imu), _obs_offsets([imu]))
    assert not r.imu_residuals[0, :, 15:].any()


def test_host_window_form_matches_batch(ctx, cfg, ocfg):
    from cerberus_amd import api
    ws = [_window(cfg, ocfg, seed=s, L=70) for s in (21, 22, 23)]
    b = _solved(ctx, ws)
    kw = dict(observations=True, imu=True)
    r = b.residuals(**kw)
    h = ctx.window_residuals(ws, **kw)
    oo = _obs_offsets(ws)
    for i in range(3):
        _bitwise(_window_part(h, i, oo), _window_part(r, i, oo))
    fresh = api.Batch(ctx, ws).residuals(**kw)
    for i in range(3):
        _bitwise(_window_part(fresh, i, oo), _window_part(r, i, oo))


def test_field_windows(ctx, cfg, ocfg):
    """The windows of tests/field_windows.py (tracks of any length in one packed wave, part-mono, outliers on the Huber branch, a
    one-factor landmark, a group of more than 64 lanes, all-mono, partial), each twice in one batch: every output against the numpy
    definition before and after a solve, the cost the solver's own, the two positions of a window bitwise the same."""
    import field_windows as FW
    from cerberus_amd import api
    ws, names = FW.batch_of(FW.field_set(cfg, ocfg, FW.BATCH_NAMES), 2 * len(FW.BATCH_NAMES))
    kw = dict(observations=True, imu=True)
    oo = _obs_offsets(ws)
    b = api.Batch(ctx, ws)
    r0 = b.residuals(**kw)
    first = {nm: names.index(nm) for nm in FW.BATCH_NAMES}
    for nm, i in first.items():
        _check_parity(r0, i, resid_ref.window_residuals(ocfg, ws[i]), oo)
    b.solve(api.default_solve_opts(True, FW.ITERS))
    summ = b.download()
    r1 = b.residuals(**kw)
    for nm, i in first.items():
        ref = resid_ref.window_residuals(ocfg, ws[i])
        _check_parity(r1, i, ref, oo)
        assert ref["n_huber_active"] >= 0.03 * ref["n_visual_blocks"] and (ref["lm_flags"] & 4).any() and not (ref["lm_flags"] & 4).all(), nm
        assert abs(r0.cost[i] - summ[i].initial_cost) <= 1e-12 * abs(summ[i].initial_cost), nm
        assert abs(r1.cost[i] - summ[i].final_cost) <= 1e-12 * abs(summ[i].final_cost), nm
        j = names.index(nm, i + 1)
        for r in (r0, r1):
            _bitwise(_window_part(r, j, oo), _window_part(r, i, oo))


def test_bad_arguments(ctx, cfg, ocfg):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    w = _window(cfg, ocfg, seed=3, L=40)
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_residuals
    wr = (T.WindowResidual * 1)()
    o = T.ResidualOpts()
    api.lib().vilo_default_residual_opts(C.byref(o))
    assert f(None, b.handle, C.byref(o), wr, None, None, None, None, None) == -2
    assert f(ctx.h, None, C.byref(o), wr, None, None, None, None, None) == -2
    assert f(ctx.h, b.handle, C.byref(o), None, None, None, None, None, None) == -2
    for bad in (-1.0, float("nan"), float("inf")):
        o.outlier_threshold_px = bad
        assert f(ctx.h, b.handle, C.byref(o), wr, None, None, None, None, None) == -2
        with pytest.raises(Exception):
            b.residuals(outlier_threshold_px=bad)
    assert f(ctx.h, b.handle, None, wr, None, None, None, None, None) == 0 and wr[0].status == 0
    d, s = w.desc(T)
    g = api.lib().vilo_window_residuals
    assert g(ctx.h, 0, C.byref(d), C.byref(s), None, wr, None, None, None, None, None) == -2
    assert g(None, 1, C.byref(d), C.byref(s), None, wr, None, None, None, None, None) == -2
    assert g(ctx.h, 1, C.byref(d), C.byref(s), None, None, None, None, None, None, None) == -2
    assert g(ctx.h, 1, C.byref(d), C.byref(s), None, wr, None, None, None, None, None) == 0
