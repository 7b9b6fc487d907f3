"""GPU (-m gpu): vilo_batch_trial_cost and vilo_window_trial_cost. The windows are tests/retract_ref.py's kinds; batches of 1, 5 and 33, and
257 for the position test; K = 1, 5 and 16. The reference is the existing calls on a twin batch: save_state -> retract(step k, alpha k) ->
residuals() -> restore_state, held at 1e-12 relative (tests/test_residuals_gpu.py's bound for costs); the oracle (tests/trial_ref.py) is
held at ten times the floor tests/test_trial_cost.py measures (TR.TRIAL_TOL)."""
import numpy as np
import pytest

import retract_ref as RR
import trial_ref as TR

pytestmark = pytest.mark.gpu

REL = 1e-12
ITERS = 4
PARTS = ("cost", "visual_cost", "prior_cost", "imu_cost")


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def kinds(cfg, ocfg):
    return {n: RR.kind_window(cfg, ocfg, n) for n in RR.LEG_KINDS + (RR.IMU_KIND,)}


def _mask_of(w, on):
    m = np.zeros(w.L, np.uint8)
    if on:
        m[1::5] = 1
    return m


def _rounds(ctx, ws, ss, blocks, al, masks=None):
    """the reference: K rounds of save_state -> retract -> residuals -> restore_state on a batch of twins; (base Residuals, [K] Residuals)"""
    from cerberus_amd import api
    b = api.Batch(ctx, [w.twin() for w in ws])
    if masks is not None:
        b.mask_landmarks(mask=np.concatenate(masks))
    base = b.residuals()
    b.save_state()
    out = []
    for k in range(ss.shape[1]):
        r = b.retract(ss[:, k], np.concatenate([bl[k] for bl in blocks]), al[:, k])
        assert (r.status == 0).all()
        out.append(b.residuals())
        b.restore_state()
    b.close()
    return base, out


def _rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


def _hold_against_rounds(t, base, rounds, tag):
    worst = 0.0
    W, K = t.cost.shape
    for i in range(W):
        for f in PARTS:
            ref = base.imu_cost[i].sum() if f == "imu_cost" else getattr(base, f)[i]
            worst = max(worst, _rel(getattr(t.base, f)[i], ref))
        assert t.base.cost_change[i] == 0.0 and t.base.status[i] == 0 and t.base.n_negative_depth[i] == base.n_negative_depth[i]
        for k in range(K):
            assert t.status[i, k] == 0, (tag, i, k, t.status[i, k])
            for f in PARTS:
                ref = rounds[k].imu_cost[i].sum() if f == "imu_cost" else getattr(rounds[k], f)[i]
                e = _rel(getattr(t, f)[i, k], ref)
                assert e <= REL, (tag, i, k, f, e)
                worst = max(worst, e)
            assert t.cost_change[i, k] == t.base.cost[i] - t.cost[i, k]
            assert t.n_negative_depth[i, k] == rounds[k].n_negative_depth[i]
    print("MEASURED %s: trial_cost against retract + residuals rounds, largest relative difference %.1e (held %.0e)" % (tag, worst, REL))
    assert worst <= REL


_cache = {}


def _run(ctx, kinds, W, K, names=RR.LEG_KINDS):
    from cerberus_amd import api
    key = (W, K, names)
    if key not in _cache:
        ws = RR.batch_of(kinds, W, names)
        ss, ls, al, blocks = TR.steps(ws, K, 1000 + W)
        b = api.Batch(ctx, ws)
        _cache[key] = dict(ws=ws, batch=b, steps=(ss, ls, al, blocks), t=b.trial_cost(ss, ls, al))
    return _cache[key]


@pytest.mark.parametrize("W,K,names", [(1, 1, RR.LEG_KINDS), (5, 5, RR.LEG_KINDS), (33, 16, RR.LEG_KINDS), (1, 5, (RR.IMU_KIND,)), (5, 16, RR.LEG_KINDS)])
def test_against_the_existing_calls(ctx, kinds, W, K, names):
    from cerberus_amd import api
    s = _run(ctx, kinds, W, K, names)
    ss, ls, al, blocks = s["steps"]
    assert np.isnan(ss).any() and api.lib().vilo_last_trial_cost_ms(ctx.h) >= 0.0
    base, rounds = _rounds(ctx, s["ws"], ss, blocks, al)
    _hold_against_rounds(s["t"], base, rounds, "W %d K %d" % (W, K))
    for i in range(W):
        assert s["t"].best[i] == TR.best_of(s["t"].status[i], s["t"].cost[i], s["t"].cost_change[i])


@pytest.mark.parametrize("W,K,names", [(5, 5, RR.LEG_KINDS), (1, 5, (RR.IMU_KIND,))])
def test_against_the_oracle(ctx, ocfg, kinds, W, K, names):
    s = _run(ctx, kinds, W, K, names)
    ss, ls, al, blocks = s["steps"]
    t, worst = s["t"], 0.0
    for i, w in enumerate(s["ws"]):
        rec, base, best, _ = TR.trial_cost(ocfg, w, ss[i], blocks[i], al[i], ctx.pose_plus)
        worst = max(worst, _rel(t.base.cost[i], base["cost"]), max(_rel(t.cost[i, k], rec["cost"][k]) for k in range(K)))
        assert list(t.status[i]) == list(rec["status"]) and list(t.n_negative_depth[i]) == list(rec["n_negative_depth"])
    print("MEASURED W %d K %d: trial_cost against the oracle %.1e (CPU floor %.1e, held %.1e)" % (W, K, worst, TR.TRIAL_MEASURED, TR.TRIAL_TOL))
    assert worst <= TR.TRIAL_TOL


def _observe(b, ws):
    """what the sequence tests read back of a batch: state and summaries, the records and prepared records, the mask"""
    summ = [bytes(x) for x in b.download()]
    st = [[a.tobytes() for a in w.state_arrays()] for w in ws]
    recs = [(b.fetch(13 if ws[0].use_leg else 16, p).tobytes(), b.fetch(15, p).tobytes(), b.fetch(10, p).tobytes()) for p in range(len(ws))]
    return summ, st, recs


def test_nothing_moves(ctx, kinds):
    from cerberus_amd import api
    opts = api.default_solve_opts(True, ITERS)
    res = []
    for call in (False, True):
        ws = RR.batch_of(kinds, 5)
        ss, ls, al, _ = TR.steps(ws, 5, 1005)
        b = api.Batch(ctx, ws)
        b.solve(opts)
        b.save_state()
        ss, ls = np.nan_to_num(ss), np.nan_to_num(ls)
        before, used = _observe(b, ws), b.device_bytes()
        if call:
            t = b.trial_cost(ss, ls, al)
            assert (t.status == 0).all()
            assert _observe(b, ws) == before and b.device_bytes() == used
        b.solve(opts)
        assert b.path()["replay"]
        res.append(_observe(b, ws))
        b.restore_state()
        res[-1] += (_observe(b, ws)[1],)   # the snapshot slot
        b.reset()
        res[-1] += (_observe(b, ws)[1],)   # the uploaded state
        b.close()
    assert res[0] == res[1]


def _record_bytes(t, i, k=None):
    return [getattr(t, f)[i].tobytes() if k is None else getattr(t, f)[i, k].tobytes() for f in TR.FIELDS]


def test_independent_of_batch_size_and_position(ctx, kinds):
    from cerberus_amd import api
    name, K = "f60_partial8", 5
    s1, _, a1, b1 = TR.steps([kinds[name]], K, 81)
    ref = None
    for W, positions in ((1, (0,)), (257, (0, 1, 63, 64, 256))):
        ws = RR.batch_of(kinds, W)
        for pos in positions:
            ws[pos] = kinds[name].twin()
        ss, ls, al, blocks = TR.steps(ws, K, 300 + W)
        for pos in positions:
            ss[pos], al[pos], blocks[pos] = s1[0], a1[0], b1[0]
        b = api.Batch(ctx, ws)
        t = b.trial_cost(ss, np.concatenate([x.ravel() for x in blocks]), al)
        b.close()
        for pos in positions:
            got = (_record_bytes(t, pos), _record_bytes(t.base, pos), int(t.best[pos]))
            if ref is None:
                ref = got
            assert got == ref, (W, pos)


def test_independent_of_the_number_of_steps(ctx, kinds):
    from cerberus_amd import api
    s = _run(ctx, kinds, 5, 16)
    ss, ls, al, blocks = s["steps"]
    b, t16 = s["batch"], s["t"]
    for k in (0, 7, 15):
        lk = np.concatenate([bl[k] for bl in blocks])
        t1 = b.trial_cost(ss[:, k:k + 1], lk, al[:, k:k + 1])
        # as column 0 of a K = 5 call, the other columns any steps
        cols = [k, 1, 2, 3, 4]
        t5 = b.trial_cost(ss[:, cols], np.concatenate([bl[cols].ravel() for bl in blocks]), al[:, cols])
        for i in range(5):
            assert _record_bytes(t16, i, k) == _record_bytes(t1, i, 0) == _record_bytes(t5, i, 0), (k, i)
            assert _record_bytes(t16.base, i) == _record_bytes(t1.base, i) == _record_bytes(t5.base, i)


@pytest.mark.parametrize("name", RR.LEG_KINDS + (RR.IMU_KIND,))
def test_directional_derivative(ctx, kinds, name):
    """K = 2 at +-RR.EPS along a unit direction: (c+ - c-) / (2 EPS) against g . d of gradient(), in units of |g|, within RR.DD_TOL"""
    from cerberus_amd import api
    w = kinds[name].twin()
    b = api.Batch(ctx, [w])
    g = b.gradient()
    ds, dl = RR.unit_direction(w, np.random.default_rng(RR.DD_SEED))
    gd = float((g.state_grad[0] * ds).sum() + (g.lm_grad * dl).sum())
    t = b.trial_cost(np.stack([ds, ds])[None], np.concatenate([dl, dl]), np.array([[RR.EPS, -RR.EPS]]))
    b.close()
    assert (t.status == 0).all()
    dd = (t.cost[0, 0] - t.cost[0, 1]) / (2.0 * RR.EPS)
    err = RR.dd_error(dd, gd, g.norm[0])
    print("MEASURED %s: |dd - g.d| / |g| = %.1e (CPU floor %.1e, held %.1e)" % (name, err, RR.DD_MEASURED, RR.DD_TOL))
    assert err <= RR.DD_TOL, (name, err)


def test_gain_ratio_wiring(ctx, kinds):
    """delta from gauss_newton_step at three mu, packed as K = 3: every cost_change has the sign of the step's model_cost_change (alpha 1,
    on the 2-frame window 1/2), and best is the arg-max of cost_change"""
    from cerberus_amd import api
    ws = RR.batch_of(kinds, 5)
    b = api.Batch(ctx, ws)
    steps = [b.gauss_newton_step(mu) for mu in (1e-8, 1e-4, 1e-2)]   # (mu = 0 is rank deficient on the 2-frame window, which has no prior)
    assert all((s.status == 0).all() for s in steps)
    ss = np.stack([s.state_step for s in steps], axis=1)
    ls = np.concatenate([np.concatenate([s.lm_step[s.offsets[i]:s.offsets[i + 1]] for s in steps]) for i in range(5)])
    al = np.ones((5, 3))
    al[RR.LEG_KINDS.index("g2")] = 0.5
    t = b.trial_cost(ss, ls, al)
    b.close()
    model = np.stack([s.model_cost_change for s in steps], axis=1)
    print("MEASURED cost_change / model_cost_change:\n%s" % (t.cost_change / model))
    assert (t.status == 0).all() and (np.sign(t.cost_change) == np.sign(model)).all() and (model > 0).all()
    assert list(t.best) == [int(np.argmax(c)) if (c > 0).any() else -1 for c in t.cost_change]


@pytest.mark.parametrize("W,K", [(5, 5), (33, 16)])
def test_masked_landmarks(ctx, kinds, W, K):
    from cerberus_amd import api
    ws = RR.batch_of(kinds, W)
    masks = [_mask_of(w, True) for w in ws]
    ss, ls, al, blocks = TR.steps(ws, K, 2000 + W, masks)
    assert np.isnan(ls).sum() == K * sum(int(m.sum()) for m in masks) > 0
    b = api.Batch(ctx, ws)
    m0, _ = b.mask_landmarks(mask=np.concatenate(masks))
    t = b.trial_cost(ss, ls, al)
    m1, _ = b.mask_landmarks(mask=np.zeros_like(m0), combine="or")   # the mask in force is the one set
    b.close()
    assert m1.tobytes() == m0.tobytes() == np.concatenate(masks).tobytes()
    assert all(np.isfinite(getattr(t, f)).all() for f in TR.FIELDS[:5])
    base, rounds = _rounds(ctx, ws, ss, blocks, al, masks)
    _hold_against_rounds(t, base, rounds, "masked W %d K %d" % (W, K))


def test_status(ctx, kinds):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    s = _run(ctx, kinds, 5, 5)
    ss, ls, al, blocks = s["steps"]
    b, t0 = s["batch"], s["t"]
    al2 = al.copy()
    al2[3, 2] = np.inf
    t = b.trial_cost(ss, ls, al2)
    assert t.status[3, 2] == T.TRIAL_NUMERIC and t.n_negative_depth[3, 2] == 0 and all(np.isnan(getattr(t, f)[3, 2]) for f in TR.FIELDS[:5])
    for i in range(5):
        assert _record_bytes(t.base, i) == _record_bytes(t0.base, i)
        for k in range(5):
            if (i, k) != (3, 2):
                assert _record_bytes(t, i, k) == _record_bytes(t0, i, k), (i, k)
    # one landmark's inverse depth stepped below zero
    w = s["ws"][1]
    bl = [x.copy() for x in blocks]
    bl[1][4, 7] = -2.0 * w.inv_depth[7] / al[1, 4]
    t = b.trial_cost(ss, np.concatenate([x.ravel() for x in bl]), al)
    assert t.n_negative_depth[1, 4] == 1 and t.n_negative_depth.sum() == 1 and not t.base.n_negative_depth.any()
    # bad arguments: nothing is written
    rec = (T.TrialRecord * 5)()
    before = bytes(rec)
    for n in (0, 17):
        assert api.lib().vilo_batch_trial_cost(ctx.h, b.handle, n, None, None, None, None, rec, None) == -2 and bytes(rec) == before
    assert api.lib().vilo_batch_trial_cost(ctx.h, b.handle, 1, None, None, None, None, None, None) == -2
    assert api.lib().vilo_window_trial_cost(ctx.h, 0, None, None, 1, None, None, None, None, rec, None) == -2


def test_samples_in_force_are_refused(ctx, cfg, ocfg):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    from test_covariance_gpu import _window
    ws = [_window(cfg, ocfg, seed=11)]
    b = api.Batch(ctx, ws)
    b.set_samples()
    rec = (T.TrialRecord * 1)()
    before = bytes(rec)
    with pytest.raises(api.ViloError, match="vilo error -5.*vilo_batch_set_samples is in force"):
        b.trial_cost(np.zeros((1, RR.NS)))
    assert api.lib().vilo_batch_trial_cost(ctx.h, b.handle, 1, None, None, None, None, rec, None) == -5 and bytes(rec) == before
    b.set_samples(False)
    assert b.trial_cost(np.zeros((1, RR.NS))).status[0] == 0
    b.close()


def test_host_window_form(ctx, kinds):
    from cerberus_amd import api
    s = _run(ctx, kinds, 5, 5)
    ss, ls, al, _ = s["steps"]
    t = api.window_trial_cost(ctx, RR.batch_of(kinds, 5), ss, ls, al)
    for f in TR.FIELDS:
        assert getattr(t, f).tobytes() == getattr(s["t"], f).tobytes() and getattr(t.base, f).tobytes() == getattr(s["t"].base, f).tobytes()
    assert t.best.tobytes() == s["t"].best.tobytes()
