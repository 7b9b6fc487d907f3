"""GPU (-m gpu): the batch query calls at every frame count from 2 to 11, on the windows of tests/frame_windows.py (the other GPU tests of
these calls see 6, 8 and 11 frames, the gyro alignment also 2). One resident batch of the leg set and one of the IMU-only set, every
window once, solved ITERS iterations; each call is held against its numpy reference at the downloaded state, through the parity check
and at the bounds of that call's own GPU test. The reference's start-up runs the frame pose by PnP and the triangulation at every frame
count while the window fills; the other calls are what the ABI offers at any frame count."""
import numpy as np
import pytest

import frame_windows as FR
import resid_ref

pytestmark = pytest.mark.gpu
KINDS = ("leg", "vins")


@pytest.fixture(scope="module")
def solved(cfg, ocfg):
    """{kind: (batch, windows at the downloaded state, names)} of the two sets, each window once, after ITERS iterations."""
    from cerberus_amd import api
    ctx = api.Context(cfg, 0)
    out = {}
    for kind, S in (("leg", FR.leg_set(cfg, ocfg)), ("vins", FR.vins_set(cfg, ocfg))):
        names, ws = list(S), list(S.values())
        b = api.Batch(ctx, ws)
        b.solve(api.default_solve_opts(True, FR.ITERS))
        summ = b.download()
        assert all((s.iterations, s.num_successful) == (FR.ITERS, FR.ITERS) for s in summ)
        out[kind] = (b, ws, names)
    out["ctx"] = ctx
    yield out
    for k in KINDS:
        out[k][0].close()
    ctx.close()


@pytest.mark.parametrize("kind", KINDS)
def test_residuals(solved, ocfg, kind):
    from test_residuals_gpu import _check_parity, _obs_offsets
    b, ws, names = solved[kind]
    r = b.residuals(observations=True, imu=True)
    oo = _obs_offsets(ws)
    for i, (w, nm) in enumerate(zip(ws, names)):
        _check_parity(r, i, resid_ref.window_residuals(ocfg, w), oo)
        assert not r.imu_residuals[i, w.F - 1:].any() and not r.imu_cost[i, w.F - 1:].any(), nm   # no interval at or beyond F - 1
        if not w.use_leg:
            assert not r.imu_residuals[i, :, 15:].any(), nm


@pytest.mark.parametrize("kind", KINDS)
def test_gradient(solved, ocfg, kind):
    from test_gradient_gpu import _check_parity
    b, ws, names = solved[kind]
    r = b.gradient()
    for i, (w, nm) in enumerate(zip(ws, names)):
        _check_parity(r, i, ocfg, w, "frame counts %s (F %d) solved" % (nm, w.F))


@pytest.mark.parametrize("kind", KINDS)
def test_triangulate(solved, kind):
    from test_triangulate_gpu import _check_parity
    b, ws, names = solved[kind]
    r = b.triangulate("all", shift=True)
    assert list(r.offsets) == np.concatenate([[0], np.cumsum([w.L for w in ws])]).tolist()
    for i, (w, nm) in enumerate(zip(ws, names)):
        _check_parity(r, i, w, "frame counts %s (F %d)" % (nm, w.F), select="all")


@pytest.mark.parametrize("kind", KINDS)
def test_frame_pose_pnp_of_the_newest_frame(solved, kind):
    """Frame F - 1, from the pose of the frame before it: what start-up asks for while the window fills."""
    import pnp_ref
    from test_pnp_gpu import _check_parity
    b, ws, names = solved[kind]
    for guess in ("previous", "current"):
        r = b.frame_pose_pnp(-1, guess, step_tolerance=pnp_ref.PARITY_STEP_TOLERANCE)
        for i, (w, nm) in enumerate(zip(ws, names)):
            _check_parity(r, i, w, "frame counts %s (F %d) frame %d %s" % (nm, w.F, w.F - 1, guess), -1, guess)


@pytest.mark.parametrize("kind", KINDS)
def test_gyro_bias_align(solved, kind):
    from test_gyro_align_gpu import LINS, _check_parity
    b, ws, names = solved[kind]
    for lin in LINS:
        r = b.gyro_bias_align(lin)
        for i, (w, nm) in enumerate(zip(ws, names)):
            _check_parity(r, i, w, "frame counts %s (F %d)" % (nm, w.F), lin)


@pytest.mark.parametrize("kind", KINDS)
def test_predict_next_frame(solved, kind):
    """The constant-velocity pose needs the two frames before the next one's predecessor: a window of 2 frames reports TOO_FEW_FRAMES, as
    the definition does, and predicts from a given pose."""
    import predict_ref
    from test_predict import given_pose
    from test_predict_gpu import _check_parity
    b, ws, names = solved[kind]
    given = np.stack([given_pose(w) for w in ws])
    for right in (False, True):
        r = b.predict_next_frame("constant_velocity", None, right)
        g = b.predict_next_frame("given", given, right)
        for i, (w, nm) in enumerate(zip(ws, names)):
            tag = "frame counts %s (F %d)%s" % (nm, w.F, " right" if right else "")
            _check_parity(r, i, w, tag, want_status=predict_ref.TOO_FEW_FRAMES if w.F < 3 else predict_ref.OK)
            _check_parity(g, i, w, tag, "given", given[i])


def _cov_class(ocfg, w, threshold=1e-14):
    """What the numpy definition itself says of the window at its state, under the frame-0 gauge: "singular" when the equilibrated
    system is not positive definite in FP64 (measured on a CPU: every window of 2 and 3 frames, leg and IMU-only: two or three frames do
    not separate the accelerometer bias from gravity), "threshold" when its reciprocal condition number is below the call's
    min_reciprocal_condition (1e-14; measured: every IMU-only window, 3.5e-17 .. 5.3e-15, as tests/test_covariance_gpu.py says of
    USE_LEG = 0 without a prior; g4 5.0e-15, g5_exfree 9.9e-15), where the definition's own FP64 floor reaches 1.8e-6, else "regular"
    (1.7e-14 .. 1.8e-13, floor 3.8e-10 .. 9.8e-9 against partial_F6's tolerance of 2e-3)."""
    import cov_ref
    H, cols, _ = cov_ref.hessian(ocfg, w)
    N = cov_ref.gauge_basis(w, cols, H.shape[0])
    A = N.T @ H @ N
    d = 1.0 / np.sqrt(np.diag(A))
    ev = np.linalg.eigvalsh(A * d[:, None] * d[None, :])
    try:
        np.linalg.cholesky(A * d[:, None] * d[None, :])
    except np.linalg.LinAlgError:
        return "singular", ev[0] / ev[-1]
    return ("threshold" if ev[0] / ev[-1] < threshold else "regular"), ev[0] / ev[-1]


def _cov_expect(ocfg, ws, names, status, kind):
    """{window index: class}; a singular window must report status 1, a regular one 0, one below the threshold either. Every frame count
    from 5 to 11 has a regular leg window."""
    out = {}
    for i, (w, nm) in enumerate(zip(ws, names)):
        c, rc = _cov_class(ocfg, w)
        print("MEASURED frame counts covariance %s (F %d): definition %s, reciprocal condition %.1e, status %d" % (nm, w.F, c, rc, status[i]))
        assert status[i] == {"singular": 1, "regular": 0}.get(c, status[i]) and status[i] in (0, 1), (nm, c, rc, status[i])
        out[i] = c
    if kind == "leg":
        assert {ws[i].F for i, c in out.items() if c == "regular"} >= set(range(5, 12))
    return out


@pytest.mark.parametrize("kind", KINDS)
def test_covariance(solved, ocfg, kind):
    """Frame blocks and the 6F-wide pose system under the frame-0 gauge, with partial_F6's options and tolerances (no prior), on every
    window the definition itself can invert (_cov_class); NaN and status 1 where it cannot."""
    import cov_ref
    from test_covariance import _floor
    rng = np.random.default_rng(5)
    b, ws, names = solved[kind]
    fr, po, st = b.covariance(gauge="frame0", poses=True)
    cls = _cov_expect(ocfg, ws, names, st, kind)
    tp, ts = cov_ref.tolerances(False)
    for i, (w, nm) in enumerate(zip(ws, names)):
        if st[i]:
            assert np.isnan(fr[i]).all() and np.isnan(po[i]).all(), nm
        if cls[i] != "regular":
            continue
        fr_r, po_r = cov_ref.window_covariance(ocfg, w, gauge="frame0")
        err = cov_ref.block_errors(fr[i], fr_r, po[i], po_r)
        # partial_F6's tolerance, or ten times this window's own FP64 floor where that is larger: the floor of the definition as
        # tests/test_covariance.py::test_fp64_floor_measured takes it (two routes, a one-ulp perturbation of J), on a CPU, numpy alone
        routes, ulp, _ = _floor(ocfg, w, "frame0", rng)
        floor = {k: max(routes[k], ulp[k]) for k in routes}
        tol = {k: max(ts if k == "sb" else tp, 10.0 * floor[k]) for k in floor}
        print("MEASURED frame counts covariance %s (F %d): %s; FP64 floor of the definition %s; held at %s"
              % (nm, w.F, {k: "%.1e" % v for k, v in err.items()}, {k: "%.1e" % v for k, v in floor.items()}, {k: "%.1e" % v for k, v in tol.items()}))
        assert all(err[k] < tol[k] for k in tol), (nm, err, tol)
        # structural zeros: absent frames, constant blocks, frame 0's position under the gauge
        assert np.all(fr[i][fr_r == 0.0] == 0.0) and np.all(po[i][po_r == 0.0] == 0.0), nm
        assert not fr[i, w.F:].any(), nm
        assert np.abs(fr[i, 0, :3, :]).max() == 0.0 and np.abs(po[i, :3, :]).max() == 0.0
        np.testing.assert_array_equal(po[i], po[i].T)


@pytest.mark.parametrize("kind", KINDS)
def test_landmark_covariance(solved, ocfg, kind):
    import lm_cov_ref
    from test_landmark_covariance import _ulp_floor
    from test_landmark_covariance_gpu import _assert_points_close, _window_slice
    rng = np.random.default_rng(9)
    b, ws, names = solved[kind]
    r = b.landmark_covariance(gauge="frame0")
    cls = _cov_expect(ocfg, ws, names, r.status, kind)
    assert r.offsets[-1] == sum(w.L for w in ws)
    for i, (w, nm) in enumerate(zip(ws, names)):
        if r.status[i]:
            assert np.isnan(r.inv_depth_var[r.offsets[i]:r.offsets[i + 1]]).all(), nm
        if cls[i] != "regular":
            continue
        # test_landmark_covariance_gpu._check_parity with the no-prior tolerances, or ten times this window's own FP64 floor where that
        # is larger (tests/test_landmark_covariance.py::test_fp64_floor_measured's one-ulp perturbation of J, on a CPU, numpy alone)
        var, pts, pc = _window_slice(r, i)
        var_r, pts_r, pc_r = lm_cov_ref.landmark_covariance(ocfg, w, gauge="frame0")
        e = lm_cov_ref.errors(var, pc, var_r, pc_r)
        floor = _ulp_floor(ocfg, w, "frame0", rng)
        tv, tp = lm_cov_ref.tolerances(False)
        tv, tp = max(tv, 10.0 * floor["var"]), max(tp, 10.0 * floor["pcov"])
        print("MEASURED frame counts landmark covariance %s (F %d): var %.1e pcov %.1e; FP64 floor of the definition var %.1e pcov %.1e; held at %.1e / %.1e"
              % (nm, w.F, e["var"], e["pcov"], floor["var"], floor["pcov"], tv, tp))
        assert e["var"] < tv and e["pcov"] < tp, (nm, e, tv, tp)
        _assert_points_close(pts, pts_r, nm)
        np.testing.assert_array_equal(pc, np.transpose(pc, (0, 2, 1)))
        assert np.all(var > 0) and np.all(np.linalg.eigvalsh(pc) > -1e-12 * np.abs(pc).max())


def _fresh_solved(solved, cfg, ocfg, kind):
    """A batch of its own for the calls that write the device state: the set at its initial state, solved ITERS iterations."""
    from cerberus_amd import api
    ws = list((FR.leg_set if kind == "leg" else FR.vins_set)(cfg, ocfg).values())
    for w in ws:
        w.uploaded_pose0 = w.pose[0].copy()
    b = api.Batch(solved["ctx"], ws)
    b.solve(api.default_solve_opts(True, FR.ITERS))
    b.download()
    return b, ws


@pytest.mark.parametrize("kind", KINDS)
def test_failure_detection_and_gauge_fix(solved, cfg, ocfg, kind):
    """failure_detection at the solved state, then gauge_fix to frame 0 as uploaded and, after a reset and the same solve, to given
    anchors; every constant extrinsic block comes back as it was."""
    from cerberus_amd import api
    from test_gauge_fix import given_anchor
    from test_gauge_fix_gpu import _check_failure, _check_gauge
    b, ws = _fresh_solved(solved, cfg, ocfg, kind)
    try:
        _check_failure(b, ws, "frame counts %s" % kind)
        _check_gauge(b, ws, None, "frame counts %s uploaded" % kind)
        b.reset()
        b.solve(api.default_solve_opts(True, FR.ITERS))
        b.download()
        _check_gauge(b, ws, np.array([given_anchor(w.uploaded_pose0, k) for k, w in enumerate(ws)]), "frame counts %s given" % kind)
    finally:
        b.close()


@pytest.mark.parametrize("kind", KINDS)
def test_dead_reckon_from_the_frame_before_the_newest(solved, cfg, ocfg, kind):
    """From frame F - 2 with write=True: frame F - 1 receives the result. from_frame is one value per call, so one call per frame count,
    each on the solved state again (the call also writes the other windows' frame f + 1, or reports NO_FRAME where they have none);
    ranges of 30, 2, 1 and 0 samples side by side."""
    import deadreckon_ref as D
    from cerberus_amd import api
    from test_dead_reckon import RANGES, take
    from test_dead_reckon_gpu import _check_parity, _pack
    b, ws = _fresh_solved(solved, cfg, ocfg, kind)
    ranges = [take(w, RANGES[::-1][i % len(RANGES)], 3 * i) for i, w in enumerate(ws)]
    samples, offsets = _pack(ranges)
    try:
        for n, f in enumerate(sorted({w.F - 2 for w in ws})):
            if n:
                b.reset()
                b.solve(api.default_solve_opts(True, FR.ITERS))
                b.download()
            before = [w.clone_state() for w in ws]
            r = b.dead_reckon(samples, offsets, f, write=True, trajectory=True)
            for i, w in enumerate(ws):
                if w.F - 2 == f:
                    _check_parity(r, i, w, ranges[i], cfg.g_norm, f, "frame counts window %d (%d frames) from_frame %d" % (i, w.F, f), write=True)
                assert r.status[i] == (D.OK if f + 1 <= w.F - 1 else D.NO_FRAME), (i, w.F, f, r.status[i])
            b.download()
            for i, w in enumerate(ws):
                want = [a.copy() for a in before[i]]
                if w.F - 2 >= f:
                    want[0][f + 1] = r.state[i, 0:7]
                    want[1][f + 1, 0:3] = r.state[i, 7:10]
                if w.F - 2 == f:
                    for x, y in zip(w.state_arrays(), want):
                        assert x.tobytes() == y.tobytes(), (i, w.F, f)
    finally:
        b.close()


def test_marginalisation_takes_full_windows_only(solved, cfg, ocfg):
    """vilo_optimize_windows on the leg set, MARGIN_OLD asked of every window: the windows of fewer than 11 frames keep valid == 0 (the
    reference marginalises full windows only, estimator.cpp:1243-1244), and the 11-frame window's prior is bit for bit the one
    vilo_marginalize gives that window alone at the state the call returned."""
    import ctypes as C
    from cerberus_amd import api, _ctypes as T
    from cerberus_amd.synth import PriorData
    ctx = solved["ctx"]
    S = FR.leg_set(cfg, ocfg)
    names, ws = list(S), list(S.values())
    W = len(ws)
    descs, states, summ, priors = (T.WindowDesc * W)(), (T.WindowState * W)(), (T.SolveSummary * W)(), (T.Prior * W)()
    out = [PriorData() for _ in ws]
    for i, w in enumerate(ws):
        descs[i], states[i] = w.desc(T)
        priors[i] = out[i].struct
    opts = api.default_solve_opts(True, FR.ITERS)
    ctx._check(api.lib().vilo_optimize_windows(ctx.h, W, descs, states, C.byref(opts), (C.c_int * W)(*([0] * W)), priors, summ))
    full = [i for i, w in enumerate(ws) if w.F == 11]
    assert [names[i] for i in full] == ["g11"]
    for i, w in enumerate(ws):
        assert (summ[i].iterations, summ[i].num_successful) == (FR.ITERS, FR.ITERS), names[i]
        assert priors[i].valid == (1 if i in full else 0), (names[i], priors[i].valid)
    i = full[0]
    got, alone = out[i], PriorData()
    got.struct = priors[i]
    ctx.marginalize(ws[i], 0, alone)
    n = got.n
    assert alone.struct.valid == 1 and alone.n == n > 0 and alone.blocks() == got.blocks()
    assert alone.J0[:n * n].tobytes() == got.J0[:n * n].tobytes() and alone.r0[:n].tobytes() == got.r0[:n].tobytes()
    assert alone.x0.tobytes() == got.x0.tobytes()
