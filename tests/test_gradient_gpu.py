"""GPU (-m gpu): vilo_batch_gradient / vilo_window_gradient against the numpy definition (tests/grad_ref.py on ref_gradient's
cost_and_gradient) at the state the device returns, stationarity after a long solve, agreement with the solver's gradient_tolerance
test, freedom from side effects, independence of batch size and position, edge windows, the host form and bad arguments.
Tolerances: ten times the FP64 floor tests/test_gradient.py measures (grad_ref.TOL_G on |dg_i| / max(sqrt(h_i), |g_i|), grad_ref.TOL_H on
|dh_i| / h_i)."""
import ctypes as C

import numpy as np
import pytest

import grad_ref
from test_covariance_gpu import CASES, _window
from test_landmark_covariance_gpu import _no_landmarks

pytestmark = pytest.mark.gpu

RECORD = ("max_norm", "norm", "scaled_max", "argmax_kind", "argmax_index", "argmax_component", "n_free", "status")


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _window_part(r, i):
    """window i's outputs, every array of them"""
    a, b = r.offsets[i], r.offsets[i + 1]
    return [np.array([getattr(r, f)[i] for f in RECORD[:3]]), np.array([getattr(r, f)[i] for f in RECORD[3:]]), r.state_grad[i],
            r.state_diag[i], r.lm_grad[a:b], r.lm_diag[a:b]]


def _bitwise(x, y):
    for a, b in zip(x, y):
        assert a.shape == b.shape
        assert a.tobytes() == b.tobytes()


def _check_parity(r, i, ocfg, w, tag):
    a, b = r.offsets[i], r.offsets[i + 1]
    got = (r.state_grad[i], r.state_diag[i], r.lm_grad[a:b], r.lm_diag[a:b])
    _, sg, sd, lg, ld, _ = grad_ref.window_gradient(ocfg, w)
    eg, eh = grad_ref.errors(w, got, (sg, sd, lg, ld))
    print("MEASURED %s: gradient %.1e (floor %.0e, tolerance %.0e), diagonal %.1e (floor %.0e, tolerance %.0e)"
          % (tag, eg, grad_ref.FLOOR_G, grad_ref.TOL_G, eh, grad_ref.FLOOR_H, grad_ref.TOL_H))
    assert eg <= grad_ref.TOL_G and eh <= grad_ref.TOL_H, (tag, eg, eh)
    free = grad_ref.free_mask(w)
    assert not got[0][~free].any() and not got[1][~free].any()   # constant blocks and absent frames: zero
    # the record, from the downloaded arrays
    rec = grad_ref.record(free, *got)
    assert r.status[i] == 0
    for f in ("max_norm", "norm", "scaled_max"):
        assert abs(getattr(r, f)[i] - rec[f]) <= 1e-14 * abs(rec[f]), (tag, f, getattr(r, f)[i], rec[f])
    for f in ("argmax_kind", "argmax_index", "argmax_component", "n_free"):
        assert getattr(r, f)[i] == rec[f], (tag, f, getattr(r, f)[i], rec[f])


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_numpy(ctx, cfg, ocfg, case):
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=401 + len(case), **CASES[case])
    b = api.Batch(ctx, [w])
    _check_parity(b.gradient(), 0, ocfg, w, case + " initial")
    b.solve(api.default_solve_opts(True, 6))
    b.download()
    _check_parity(b.gradient(), 0, ocfg, w, case + " solved")


def test_stationarity(ctx, cfg, ocfg):
    from cerberus_amd import api
    ws = [_window(cfg, ocfg, seed=s, L=60) for s in (41, 42, 43)]
    b = api.Batch(ctx, ws)
    start = b.gradient(state=False, landmarks=False).scaled_max.copy()
    b.solve(api.default_solve_opts(True, 40))
    end = b.gradient(state=False, landmarks=False).scaled_max
    print("MEASURED scaled_max:", ["%.1e -> %.1e" % (s, e) for s, e in zip(start, end)])
    assert (end <= 1e-8 * start).all(), (start, end)


@pytest.mark.parametrize("form", ["auto", "wave"])
def test_max_norm_is_what_gradient_tolerance_reads(ctx, cfg, ocfg, form):
    """The solver forms their gmax (max |g_i|, unscaled, over the free camera dimensions and the inverse depths) in another order of the
    sums; the forms agree to 4e-10, the margin is 1e-6."""
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=51, L=60)
    ctx.set_solver_form(form)
    try:
        gmax = api.Batch(ctx, [w.twin()]).gradient().max_norm[0]
        out = []
        for f in (1.0 + 1e-6, 1.0 - 1e-6):
            o = api.default_solve_opts(False, 3)
            o.gradient_tolerance = gmax * f
            b = api.Batch(ctx, [w.twin()])
            b.solve(o)
            s = b.download()[0]
            out.append((s.termination, s.num_successful, s.final_cost == s.initial_cost))
        assert out[0] == (1, 0, True), out
        assert not (out[1][0] == 1 and out[1][1] == 0), out
    finally:
        ctx.set_solver_form("auto")


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
        b.gradient()
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


def test_device_memory_is_returned(ctx, cfg, ocfg):
    from cerberus_amd import api
    b = api.Batch(ctx, [_window(cfg, ocfg, seed=s, L=50) for s in (13, 14)])
    first = b.gradient()
    bytes0 = b.device_bytes()
    for _ in range(5):
        r = b.gradient()
        assert b.device_bytes() == bytes0
    for i in range(2):
        _bitwise(_window_part(r, i), _window_part(first, i))


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg):
    """300 windows of 200 landmarks cross the 256-packed-wave boundary of the visual linearisation's forms."""
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=77, L=200)
    other = _window(cfg, ocfg, seed=78, L=200)
    alone = _window_part(api.Batch(ctx, [w.twin()]).gradient(), 0)
    eight = [other.twin() for _ in range(8)]
    eight[3] = w.twin()
    _bitwise(_window_part(api.Batch(ctx, eight).gradient(), 3), alone)
    for pos in (0, 150, 299):
        many = [other.twin() for _ in range(300)]
        many[pos] = w.twin()
        b = api.Batch(ctx, many)
        _bitwise(_window_part(b.gradient(), pos), alone)
        b.close()


def test_edge_windows(ctx, cfg, ocfg):
    from cerberus_amd import api
    e0 = _no_landmarks(_window(cfg, ocfg, seed=62, L=10))
    r = api.Batch(ctx, [e0.twin()]).gradient(landmarks=False)   # landmark buffers NULL
    assert r.lm_grad is None and r.status[0] == 0 and r.n_free[0] == int(grad_ref.free_mask(e0).sum())
    nop = _window(cfg, ocfg, seed=63, L=40, prior=False)
    f6 = _window(cfg, ocfg, seed=64, L=40, F=6, prior=False, leg_bias_const=1)
    cst = _window(cfg, ocfg, seed=67, L=40, ex_const=1, td_const=1, leg_bias_const=1)
    bad = _window(cfg, ocfg, seed=65, L=40)
    bad.preint = bad.preint.copy()
    bad.preint[2][33 + 961] = -1.0   # covariance (0, 0) of interval 2: not positive definite, no sqrt_info
    ws = [e0, nop, bad, f6, cst]
    r = api.Batch(ctx, [w.twin() for w in ws]).gradient()
    assert list(r.offsets) == [0, 0, 40, 80, 80 + f6.L, 80 + f6.L + 40]
    for i, w in ((0, e0), (1, nop), (3, f6), (4, cst)):
        _check_parity(r, i, ocfg, w, "edge %d" % i)
        alone = api.Batch(ctx, [w.twin()]).gradient()
        _bitwise(_window_part(r, i), _window_part(alone, 0))
    # n_frames = 6: the rows of frames 6 .. 10 are zero; 6 poses, 6 speed-bias blocks, both extrinsics, the landmarks
    assert not r.state_grad[3, 36:66].any() and not r.state_grad[3, 66 + 54:165].any() and not r.state_grad[3, 165:209].any()
    assert r.n_free[3] == 6 * 6 + 6 * 9 + 12 + f6.L
    # ex_const, td_const, leg_bias_const: zero rows, 11 poses and speed-bias blocks left
    assert not r.state_grad[4, 165:].any() and not r.state_diag[4, 165:].any() and r.n_free[4] == 11 * 15 + 40
    # a record without sqrt_info: status 2 and NaN, for that window only
    assert r.status[2] == 2 and np.isnan(r.max_norm[2]) and np.isnan(r.norm[2]) and np.isnan(r.scaled_max[2])
    assert np.isnan(r.state_grad[2]).all() and np.isnan(r.state_diag[2]).all()
    assert np.isnan(r.lm_grad[40:80]).all() and np.isnan(r.lm_diag[40:80]).all()
    assert np.isfinite(np.delete(r.state_grad, 2, axis=0)).all() and np.isfinite(np.delete(r.lm_grad, np.arange(40, 80))).all()
    # USE_LEG = 0 (a batch of its own: one IMU factor kind per batch): no leg-bias coordinates
    imu = _window(cfg, ocfg, seed=66, L=40, use_leg=0, leg_bias_const=1)
    r = api.Batch(ctx, [imu.twin()]).gradient()
    _check_parity(r, 0, ocfg, imu, "use_leg 0")
    assert not r.state_grad[0, 165:209].any() and r.n_free[0] == 11 * 15 + 12 + 40


def test_field_windows(ctx, cfg, ocfg):
    """The windows of tests/field_windows.py, each twice in one batch: gradient and Gauss-Newton diagonal against the numpy definition
    at the measured-floor bounds, before and after a solve; the two positions of a window bitwise the same."""
    import field_windows as FW
    from cerberus_amd import api
    ws, names = FW.batch_of(FW.field_set(cfg, ocfg, FW.BATCH_NAMES), 2 * len(FW.BATCH_NAMES))
    b = api.Batch(ctx, ws)
    for stage in ("initial", "solved"):
        if stage == "solved":
            b.solve(api.default_solve_opts(True, FW.ITERS))
            b.download()
        r = b.gradient()
        for nm in FW.BATCH_NAMES:
            i = names.index(nm)
            _check_parity(r, i, ocfg, ws[i], "field %s %s" % (nm, stage))
            _bitwise(_window_part(r, names.index(nm, i + 1)), _window_part(r, i))


def test_host_window_form_matches_batch(ctx, cfg, ocfg):
    from cerberus_amd import api
    ws = [_window(cfg, ocfg, seed=s, L=70) for s in (21, 22, 23)]
    b = api.Batch(ctx, ws)
    b.solve(api.default_solve_opts(True, 6))
    b.download()
    r = b.gradient()
    h = ctx.window_gradient(ws)
    for i in range(3):
        _bitwise(_window_part(h, i), _window_part(r, i))


def test_bad_arguments(ctx, cfg, ocfg):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    w = _window(cfg, ocfg, seed=3, L=40)
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_gradient
    wg = (T.WindowGradient * 1)()
    assert f(None, b.handle, wg, None, None, None, None) == -2
    assert f(ctx.h, None, wg, None, None, None, None) == -2
    assert f(ctx.h, b.handle, None, None, None, None, None) == -2
    assert f(ctx.h, b.handle, wg, None, None, None, None) == 0 and wg[0].status == 0 and wg[0].n_free == 11 * 19 + 12 + 40
    assert api.lib().vilo_last_gradient_ms(ctx.h) > 0.0
    d, s = w.desc(T)
    g = api.lib().vilo_window_gradient
    assert g(ctx.h, 0, C.byref(d), C.byref(s), wg, None, None, None, None) == -2
    assert g(None, 1, C.byref(d), C.byref(s), wg, None, None, None, None) == -2
    assert g(ctx.h, 1, C.byref(d), C.byref(s), None, None, None, None, None) == -2
    assert g(ctx.h, 1, C.byref(d), C.byref(s), wg, None, None, None, None) == 0
