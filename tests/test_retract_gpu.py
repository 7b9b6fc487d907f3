"""GPU (-m gpu): vilo_batch_retract, vilo_batch_set_state, vilo_batch_save_state / _restore_state and vilo_window_retract.
The windows are tests/retract_ref.py's kinds (twins of field_windows / const_windows / frame_windows windows): 8 frames with ragged tracks, a
free td, constant extrinsics, constant leg biases, 2 frames, and an IMU-only window in a batch of its own; batches of 1, 5 and 33, and 257
for the position test. The stepped state is compared byte for byte with the numpy restatement (additive blocks) and Context.pose_plus (pose
and extrinsic blocks); the directional-derivative tolerance is ten times what tests/test_retract.py measures with the oracle alone."""
import numpy as np
import pytest

import retract_ref as RR

pytestmark = pytest.mark.gpu

ITERS = 4


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kinds(cfg, ocfg):
    """{name: window}: never uploaded, so each keeps its start state; the tests work on twins"""
    return {n: RR.kind_window(cfg, ocfg, n) for n in RR.LEG_KINDS + (RR.IMU_KIND,)}


def _bytes(ws):
    return [[a.tobytes() for a in w.state_arrays()] for w in ws]


def _mask_of(w, on):
    m = np.zeros(w.L, np.uint8)
    if on:
        m[1::5] = 1
    return m


def _steps(ws, seed, masks=None):
    """random steps of size 1e-2 with NaN wherever the call must not read, and an alpha per window in [0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    ss, ls = zip(*[RR.random_step(w, rng, lm_mask=None if masks is None else masks[i]) for i, w in enumerate(ws)])
    return np.array(ss), list(ls), 0.5 + rng.random(len(ws))


def _expected(ctx, ws, ss, ls, alpha, masks=None):
    """[(state arrays, record)] of the numpy restatement on the windows' current arrays, the pose blocks through Context.pose_plus"""
    return [RR.retract(w, ss[i], ls[i], alpha[i], ctx.pose_plus, lm_mask=None if masks is None else masks[i]) for i, w in enumerate(ws)]


def _check_records(r, exp, tag):
    for i, (_, rec) in enumerate(exp):
        assert r.status[i] == rec["status"] and r.n_applied[i] == rec["n_applied"], (tag, i, r.status[i], r.n_applied[i], rec)
        un, um = RR.ulps(r.step_norm[i], rec["step_norm"]), RR.ulps(r.step_max[i], rec["step_max"])
        assert un <= 4 and um <= 4, (tag, i, un, um)


def _check_states(ws, exp, tag):
    for i, (w, (arrs, _)) in enumerate(zip(ws, exp)):
        for k, (a, e) in enumerate(zip(w.state_arrays(), arrs)):
            assert a.tobytes() == e.tobytes(), (tag, "window", i, "array", k, float(np.nanmax(np.abs(a - e))) if a.size else 0.0)


_cache = {}


def _stepped(ctx, kinds, W, names=RR.LEG_KINDS):
    """Test 1's run at W windows, once per module: the batch after the step (not downloaded again), its windows holding the downloaded
    state, what the restatement expected, the steps"""
    from cerberus_amd import api
    key = (W, names)
    if key not in _cache:
        ws = RR.batch_of(kinds, W, names)
        ss, ls, alpha = _steps(ws, 100 + W)
        exp = _expected(ctx, ws, ss, ls, alpha)
        b = api.Batch(ctx, ws)
        r = b.retract(ss, np.concatenate(ls), alpha)
        b.download()
        _cache[key] = dict(batch=b, ws=ws, exp=exp, rec=r, steps=(ss, ls, alpha))
    return _cache[key]


@pytest.mark.parametrize("W,names", [(1, RR.LEG_KINDS), (5, RR.LEG_KINDS), (33, RR.LEG_KINDS), (1, (RR.IMU_KIND,))])
def test_bitwise_against_the_host_restatement(ctx, kinds, W, names):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    s = _stepped(ctx, kinds, W, names)
    _check_states(s["ws"], s["exp"], "W %d" % W)
    _check_records(s["rec"], s["exp"], "W %d" % W)
    assert (s["rec"].status == T.RETRACT_OK).all() and api.lib().vilo_last_retract_ms(ctx.h) >= 0.0
    assert np.isnan(s["steps"][0]).any()   # constant blocks or absent frames: NaN was in the step there
    # with masked landmarks, NaN in their steps
    ws = RR.batch_of(kinds, W, names)
    masks = [_mask_of(w, i % 2 == 0) for i, w in enumerate(ws)]
    ss, ls, alpha = _steps(ws, 200 + W, masks)
    assert np.isnan(np.concatenate(ls)).sum() == sum(int(m.sum()) for m in masks) > 0
    exp = _expected(ctx, ws, ss, ls, alpha, masks)
    b = api.Batch(ctx, ws)
    b.mask_landmarks(mask=np.concatenate(masks))
    r = b.retract(ss, np.concatenate(ls), alpha)
    b.download()
    _check_states(ws, exp, "masked W %d" % W)
    _check_records(r, exp, "masked W %d" % W)
    # NULL steps: nothing moves but the quaternions' normalisation; the count is the same
    before = [RR.retract(w, np.zeros(RR.NS), np.zeros(w.L), 1.0, ctx.pose_plus, lm_mask=masks[i]) for i, w in enumerate(ws)]
    r0 = b.retract()
    b.download()
    _check_states(ws, before, "zero step W %d" % W)
    assert (r0.n_applied == r.n_applied).all() and not r0.step_norm.any() and not r0.step_max.any()


def _rel_states(a_list, b_list, F):
    worst = 0.0
    for i, (a, b) in enumerate(zip(a_list, b_list)):
        if a.size == 0:
            continue
        if i < 3:
            a, b = a[:F], b[:F]
        worst = max(worst, float(np.abs(a - b).max() / max(1.0, np.abs(b).max())))
    return worst


@pytest.mark.parametrize("W,form", [(5, "wave"), (33, "mw8"), (33, "split")])
def test_batch_behaves_as_a_fresh_batch_at_the_stepped_state(ctx, ocfg, kinds, W, form):
    from cerberus_amd import api
    from oracle import oracle_py as O
    s = _stepped(ctx, kinds, W)
    opts = api.default_solve_opts(True, ITERS)
    ctx.set_solver_form(form)
    try:
        # A: the batch of test 1's recipe, stepped on the device; B: a fresh batch whose host state is test 1's downloaded result
        wa = RR.batch_of(kinds, W)
        ss, ls, alpha = s["steps"]
        A = api.Batch(ctx, wa)
        A.retract(ss, np.concatenate(ls), alpha)
        wb = [w.twin() for w in s["ws"]]
        stepped = _bytes(wb)
        B = api.Batch(ctx, wb)
        ca, cb = A.residuals().cost, B.residuals().cost
        assert ca.tobytes() == cb.tobytes()
        A.save_state()
        A.solve(opts)
        assert A.path()["solver"] == form and not A.path()["replay"]
        sa = [bytes(x) for x in A.download()]
        first = _bytes(wa)
        B.solve(opts)
        sb = [bytes(x) for x in B.download()]
        assert first == _bytes(wb) and sa == sb
        # the oracle from the stepped state, each kind once
        summ = A.download()
        for i, name in enumerate(RR.LEG_KINDS):
            t = s["ws"][i].twin()
            so = O.solve_window(ocfg, t, O.default_opts(True, ITERS))
            sm = summ[i]
            e = _rel_states(wa[i].state_arrays(), t.state_arrays(), t.F)
            print("MEASURED %s W %d %s: states %.1e, cost %.1e against the oracle; successful steps %d (oracle %d)"
                  % (name, W, form, e, abs(sm.final_cost / so.final_cost - 1), sm.num_successful, so.num_successful))
            assert e < 1e-8 and abs(sm.final_cost - so.final_cost) <= 1e-8 * abs(so.final_cost), (name, e, sm.final_cost, so.final_cost)
        # the same solve again from the snapshot: a replay of the captured launch sequence, bitwise the first
        A.restore_state()
        A.download()
        assert _bytes(wa) == stepped
        A.solve(opts)
        assert A.path()["replay"]
        assert [bytes(x) for x in A.download()] == sa and _bytes(wa) == first
    finally:
        ctx.set_solver_form("auto")


@pytest.mark.parametrize("name", RR.LEG_KINDS + (RR.IMU_KIND,))
def test_layout_is_the_gradients(ctx, kinds, name):
    """Central difference of residuals().cost along a unit direction over the free coordinates against g . d of gradient(), in units of
    |g|: RR.DD_TOL, ten times what tests/test_retract.py measures with the oracle's cost and numpy's gradient. Then one preconditioned step
    -g / h, alpha halved from 1 until the cost falls."""
    from cerberus_amd import api
    w = kinds[name].twin()
    b = api.Batch(ctx, [w])
    g = b.gradient()
    assert g.status[0] == 0
    ds, dl = RR.unit_direction(w, np.random.default_rng(RR.DD_SEED))
    gd = float((g.state_grad[0] * ds).sum() + (g.lm_grad * dl).sum())
    b.save_state()

    def cost_after(step_s, step_l):
        def at(alpha):
            b.restore_state()
            r = b.retract(step_s[None], step_l, np.array([alpha]))
            assert r.status[0] == 0
            return float(b.residuals().cost[0])
        return at

    dd = RR.central_difference(cost_after(ds, dl), RR.EPS)
    err = RR.dd_error(dd, gd, g.norm[0])
    print("MEASURED %s: |dd - g.d| / |g| = %.1e (CPU floor %.1e, held %.1e; g.d %.6e, dd %.6e)" % (name, err, RR.DD_MEASURED, RR.DD_TOL, gd, dd))
    assert err <= RR.DD_TOL, (name, err)
    b.restore_state()
    c0 = float(b.residuals().cost[0])
    fs, _ = RR.applied(w)
    with np.errstate(divide="ignore", invalid="ignore"):
        ps, pl = np.where(fs & (g.state_diag[0] > 0), -g.state_grad[0] / g.state_diag[0], 0.0), np.where(g.lm_diag > 0, -g.lm_grad / g.lm_diag, 0.0)
    at = cost_after(ps, pl)
    halvings = next((k for k in range(21) if at(0.5 ** k) < c0), None)
    print("MEASURED %s: preconditioned step accepted after %s halvings" % (name, halvings))
    assert halvings is not None and halvings <= 20, name


@pytest.mark.parametrize("solved", [False, True])
def test_base_uploaded_is_reset_then_retract(ctx, kinds, solved):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    wa, wb = RR.batch_of(kinds, 5), RR.batch_of(kinds, 5)
    ss, ls, alpha = _steps(wa, 41)
    alpha[3] = np.inf   # a window that is not stepped: with UPLOADED it is reset all the same
    A, B = api.Batch(ctx, wa), api.Batch(ctx, wb)
    if solved:
        for b in (A, B):
            b.solve(api.default_solve_opts(True, ITERS))
    ra = A.retract(ss, np.concatenate(ls), alpha, base="uploaded")
    B.reset()
    rb = B.retract(ss, np.concatenate(ls), alpha)
    A.download(), B.download()
    assert _bytes(wa) == _bytes(wb)
    for f in api.Retraction._fields:
        assert getattr(ra, f).tobytes() == getattr(rb, f).tobytes()
    assert list(ra.status) == [0, 0, 0, T.RETRACT_NUMERIC, 0]
    assert _bytes(wa)[3] == _bytes([kinds[RR.LEG_KINDS[3]]])[0]   # the uploaded state
    # and the stepped windows are the restatement's result from the uploaded state
    exp = _expected(ctx, RR.batch_of(kinds, 5), ss, ls, alpha)
    _check_states(wa, exp, "uploaded")


@pytest.mark.parametrize("what", ["nan_step", "nan_landmark_step", "inf_alpha"])
def test_non_finite_steps(ctx, kinds, what):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    ws = RR.batch_of(kinds, 5)
    ss, ls, alpha = _steps(ws, 51)
    if what == "nan_step":
        ss[2, 66 + 4] = np.nan        # frame 0's accelerometer bias: applied in every window
    elif what == "nan_landmark_step":
        ls[2][ws[2].L - 1] = np.nan
    else:
        alpha[2] = np.inf
    exp = _expected(ctx, ws, ss, ls, alpha)
    assert [e[1]["status"] for e in exp] == [0, 0, T.RETRACT_NUMERIC, 0, 0]
    before = _bytes(ws)
    b = api.Batch(ctx, ws)
    r = b.retract(ss, np.concatenate(ls), alpha)
    b.download()
    assert _bytes(ws)[2] == before[2] and r.status[2] == T.RETRACT_NUMERIC and r.n_applied[2] == 0
    _check_states(ws, exp, what)
    _check_records(r, exp, what)


def test_set_state(ctx, kinds):
    from cerberus_amd import api
    ws = RR.batch_of(kinds, 5)
    start = _bytes(ws)
    b = api.Batch(ctx, ws)
    b.solve(api.default_solve_opts(True, ITERS))
    b.download()
    solved = _bytes(ws)
    rng = np.random.default_rng(61)
    new = {i: ws[i].twin() for i in (0, 3)}
    for t in new.values():
        for a in t.state_arrays():
            a += 1e-3 * rng.normal(size=a.shape)
    b.set_state([3, 0], [new[3], new[0]])
    b.download()
    for i in range(5):
        if i in new:
            F = ws[i].F
            for k, (a, e) in enumerate(zip(ws[i].state_arrays(), new[i].state_arrays())):
                assert (a[:F] if k < 3 else a).tobytes() == (e[:F] if k < 3 else e).tobytes(), (i, k)
        else:
            assert _bytes([ws[i]])[0] == solved[i], i
    now = _bytes(ws)
    for ids in ([0, 0], [1, 5], [-1, 2]):
        with pytest.raises(api.ViloError, match="vilo error -2"):
            b.set_state(ids, [new[0], new[3]])
        b.download()
        assert _bytes(ws) == now
    assert api.lib().vilo_batch_set_state(ctx.h, b.handle, 0, None, None) == -2
    b.reset()
    b.download()
    assert _bytes(ws) == start


def test_save_and_restore_state(ctx, kinds):
    from cerberus_amd import api
    ws = RR.batch_of(kinds, 5)
    b = api.Batch(ctx, ws)
    with pytest.raises(api.ViloError, match="vilo error -5.*no state has been saved"):
        b.restore_state()
    ss, ls, alpha = _steps(ws, 71)
    ss, ls = np.nan_to_num(ss), np.nan_to_num(np.concatenate(ls))
    b.retract(ss, ls, alpha)
    b.mask_landmarks(mask=np.concatenate([_mask_of(w, True) for w in ws]))   # a masked landmark's inverse depth is saved and restored like any other
    b.download()
    saved = _bytes(ws)
    bytes0 = b.device_bytes()
    b.save_state()
    bytes1 = b.device_bytes()
    assert bytes1[1] > bytes0[1]
    b.solve(api.default_solve_opts(True, ITERS))
    b.download()
    assert _bytes(ws) != saved
    b.restore_state()
    b.download()
    assert _bytes(ws) == saved
    b.save_state()
    for _ in range(3):
        b.retract(ss, ls, alpha)
        assert b.device_bytes() == bytes1
    b.restore_state()
    b.download()
    assert _bytes(ws) == saved and b.device_bytes() == bytes1


def test_independent_of_batch_size_and_position(ctx, kinds):
    from cerberus_amd import api
    name = "f60_partial8"
    rng = np.random.default_rng(81)
    s1, l1 = RR.random_step(kinds[name], rng)
    a1 = 0.75
    ref = None
    for W in (1, 33, 257):
        for pos in sorted({0, W // 2, W - 1}):
            ws = RR.batch_of(kinds, W)
            ws[pos] = kinds[name].twin()
            ss, ls, alpha = _steps(ws, 300 + W)
            ss[pos], ls[pos], alpha[pos] = s1, l1, a1
            b = api.Batch(ctx, ws)
            r = b.retract(ss, np.concatenate(ls), alpha)
            b.download()
            got = (_bytes([ws[pos]])[0], [getattr(r, f)[pos].tobytes() for f in api.Retraction._fields])
            b.close()
            if ref is None:
                ref = got
            assert got == ref, (W, pos)


def test_host_window_form(ctx, kinds):
    from cerberus_amd import api
    s = _stepped(ctx, kinds, 5)
    ws = RR.batch_of(kinds, 5)
    ss, ls, alpha = s["steps"]
    r = ctx.window_retract(ws, ss, np.concatenate(ls), alpha)
    assert _bytes(ws) == _bytes(s["ws"])
    for f in api.Retraction._fields:
        assert getattr(r, f).tobytes() == getattr(s["rec"], f).tobytes()
