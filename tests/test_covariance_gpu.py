"""GPU (-m gpu): vilo_batch_covariance / vilo_window_covariance against the numpy definition (tests/cov_ref.py on ref_gradient's dense
Jacobian at the state the device returns), rank deficiency, freedom from side effects on the batch, and independence of batch size and
position. Tolerances per entry, correlation-scaled (|dS_ij| / sqrt(S_ii S_jj)), cov_ref.tolerances: ten times the FP64 floor
tests/test_covariance.py measures (with a prior: dp dtheta / extrinsic / td 4e-5, speed-bias / rho rows 2e-4; without a prior 2e-3)."""
import ctypes as C

import numpy as np
import pytest

import cov_ref
from oracle import oracle_py as O

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _window(cfg, ocfg, seed=20260925, L=120, prior=True, ex_const=0, td_const=1, use_leg=1, leg_bias_const=0, F=11):
    from cerberus_amd import synth
    w = synth.make_window(cfg, params=synth.default_params(n_landmarks=L, seed=seed, with_prior=prior))
    O.fill_preint(ocfg, w)
    w.ex_const, w.td_const, w.use_leg, w.leg_bias_const = ex_const, td_const, use_leg, leg_bias_const
    if F < 11:
        from test_gpu_parity import _truncate
        _truncate(w, F)
        w.leg_bias_const = leg_bias_const
    return w


def _solved(ctx, windows, iters=6):
    from cerberus_amd import api
    b = api.Batch(ctx, windows)
    b.solve(api.default_solve_opts(True, iters))
    b.download()
    return b


CASES = {
    "prior": dict(),
    "no_prior": dict(prior=False),
    "ex_const": dict(ex_const=1),
    "td_free": dict(td_const=0),
    # (USE_LEG = 0 without a prior leaves a direction at a scaled eigenvalue of 3e-15, rank deficient by the definition's threshold; the
    # synthetic prior carries leg-bias blocks, held constant here as a USE_LEG = 0 window has none to estimate)
    "imu_only": dict(use_leg=0, leg_bias_const=1),
    "leg_bias_const": dict(leg_bias_const=1),
    "partial_F6": dict(F=6, prior=False, leg_bias_const=1),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_numpy(ctx, cfg, ocfg, case):
    w = _window(cfg, ocfg, seed=101 + len(case), **CASES[case])
    b = _solved(ctx, [w])
    gauges = ["frame0", "none"] if w.prior.struct.valid else ["frame0"]
    for g in gauges:
        fr, po, st = b.covariance(gauge=g, poses=True)
        assert st[0] == 0, (case, g, st)
        fr_r, po_r = cov_ref.window_covariance(ocfg, w, gauge=g)
        err = cov_ref.block_errors(fr[0], fr_r, po[0], po_r)
        tp, ts = cov_ref.tolerances(bool(w.prior.struct.valid))
        assert err["pose"] < tp and err["ex_td"] < tp and err["sb"] < ts, (case, g, err)
        # structural zeros: absent frames, constant blocks, frame 0's position under FRAME0
        assert np.all(fr[0][fr_r == 0.0] == 0.0) and np.all(po[0][po_r == 0.0] == 0.0), (case, g)
        if g == "frame0":
            assert np.abs(fr[0, 0, :3, :]).max() == 0.0 and np.abs(po[0, :3, :]).max() == 0.0
        np.testing.assert_array_equal(po[0], po[0].T)


def test_field_windows(ctx, cfg, ocfg):
    """The windows of tests/field_windows.py, each twice in one solved batch: frame blocks and the pose system against the numpy
    definition at test_parity_with_numpy's tolerances; the two positions of a window bitwise the same."""
    import field_windows as FW
    ws, names = FW.batch_of(FW.field_set(cfg, ocfg, FW.BATCH_NAMES), 2 * len(FW.BATCH_NAMES))
    b = _solved(ctx, ws, iters=FW.ITERS)
    fr, po, st = b.covariance(gauge="frame0", poses=True)
    for nm in FW.BATCH_NAMES:
        i = names.index(nm)
        w = ws[i]
        assert st[i] == 0, (nm, st)
        fr_r, po_r = cov_ref.window_covariance(ocfg, w, gauge="frame0")
        err = cov_ref.block_errors(fr[i], fr_r, po[i], po_r)
        tp, ts = cov_ref.tolerances(bool(w.prior.struct.valid))
        print("MEASURED covariance of field window %s: %s (tolerances %.0e / %.0e)" % (nm, {k: "%.1e" % v for k, v in err.items()}, tp, ts))
        assert err["pose"] < tp and err["ex_td"] < tp and err["sb"] < ts, (nm, err)
        assert np.all(fr[i][fr_r == 0.0] == 0.0) and np.all(po[i][po_r == 0.0] == 0.0), nm
        j = names.index(nm, i + 1)
        np.testing.assert_array_equal(fr[j], fr[i]); np.testing.assert_array_equal(po[j], po[i])


def test_rank_deficiency_is_per_window(ctx, cfg, ocfg):
    wp = _window(cfg, ocfg, seed=5)
    wn = _window(cfg, ocfg, seed=6, prior=False)
    b = _solved(ctx, [wp.twin(), wn.twin(), wp.twin()])
    fr, po, st = b.covariance(gauge="none", poses=True)
    assert list(st) == [0, 1, 0]
    assert np.isnan(fr[1]).all() and np.isnan(po[1]).all()
    fr0, po0, st0 = b.covariance(gauge="frame0", poses=True)
    assert list(st0) == [0, 0, 0] and np.isfinite(fr0).all()
    alone = _solved(ctx, [wp.twin()])
    fa, pa, sa = alone.covariance(gauge="none", poses=True)
    assert sa[0] == 0
    np.testing.assert_array_equal(fr[0], fa[0])
    np.testing.assert_array_equal(fr[2], fa[0])
    np.testing.assert_array_equal(po[2], pa[0])


def _hip_free_bytes():
    try:
        hip = C.CDLL("libamdhip64.so")
    except OSError:
        hip = C.CDLL("/opt/rocm/lib/libamdhip64.so")
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return free.value


def test_no_side_effects(ctx, cfg, ocfg):
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)
    # reference run: solve, solve again
    ws_a = [w.twin() for w in base]
    a = api.Batch(ctx, ws_a)
    a.solve(opts)
    a.download()
    a.solve(opts)
    summ_a = a.download()
    # the same with the covariance between the two solves
    ws_b = [w.twin() for w in base]
    b = api.Batch(ctx, ws_b)
    b.solve(opts)
    summ0 = b.download()
    before = [s.copy() for w in ws_b for s in w.state_arrays()]
    b.covariance(poses=True)
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
    # repeated calls do not grow device memory
    b.covariance(poses=True)
    free0 = _hip_free_bytes()
    for _ in range(20):
        b.covariance(poses=True)
    assert free0 - _hip_free_bytes() < (1 << 20)   # (one call's buffer for these two windows is ~0.6 MB: twenty would be 12 MB)


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg):
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=77, L=80)
    other = _window(cfg, ocfg, seed=78, L=80)
    b1 = _solved(ctx, [w.twin()], iters=3)
    ref, ref_p, _ = b1.covariance(poses=True)
    x = [a.copy() for a in b1.windows[0].state_arrays()]
    w.set_state(x)
    for W in (128, 1024, 4096):
        for pos in (0, W // 2 + 1, W - 1):
            ws = [other.twin() for _ in range(W)]
            ws[pos] = w.twin()
            bb = api.Batch(ctx, ws)   # windows at their (given) states: the covariance is evaluated there
            fr, po, st = bb.covariance(poses=True)
            assert st[pos] == 0
            np.testing.assert_array_equal(fr[pos], ref[0], err_msg="W=%d pos=%d" % (W, pos))
            np.testing.assert_array_equal(po[pos], ref_p[0])
            bb.close()
            if W == 4096:
                break


def test_host_window_form_matches_batch(ctx, cfg, ocfg):
    ws = [_window(cfg, ocfg, seed=s) for s in (21, 22, 23)]
    b = _solved(ctx, ws)
    fr, po, st = b.covariance(poses=True)
    fh, ph, sh = ctx.window_covariance(ws, poses=True)
    assert list(st) == list(sh) == [0, 0, 0]
    np.testing.assert_allclose(fh, fr, rtol=1e-12, atol=1e-14 * np.abs(fr).max())
    np.testing.assert_allclose(ph, po, rtol=1e-12, atol=1e-14 * np.abs(po).max())


def test_bad_arguments(ctx, cfg, ocfg):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    b = _solved(ctx, [_window(cfg, ocfg, seed=3, L=40)], iters=2)
    with pytest.raises(ValueError):
        b.covariance(gauge="world")
    o = api.default_cov_opts()
    o.want_poses = 1
    fr, st = np.zeros((1, 11, 19, 19)), np.zeros(1, np.int32)
    assert api.lib().vilo_batch_covariance(ctx.h, b.handle, C.byref(o), T.dptr(fr), None, T.iptr(st)) == -2
    o.want_poses, o.gauge = 0, 7
    assert api.lib().vilo_batch_covariance(ctx.h, b.handle, C.byref(o), T.dptr(fr), None, T.iptr(st)) == -2
