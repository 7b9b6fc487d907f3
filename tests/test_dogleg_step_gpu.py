"""GPU (-m gpu): vilo_batch_dogleg_step / vilo_window_dogleg_step against the numpy definition (tests/dogleg_ref.py) at dogleg_ref.TOL —
ten times the FP64 floors tests/test_dogleg_step.py measures — on every branch of every case under both gauges, at radii chosen from the
reference alone (2 |p^_gn|, alpha |g^| / 2, (alpha |g^| + |p^_gn|) / 2); branch 0 bitwise the Gauss-Newton step call's; |p^| = Delta on
branches 1 and 2; model_cost_change against the Hessian-vector call's; one caller-driven trust-region iteration against the solver's and
the oracle's; the tie to the oracle's trajectory; bitwise independence of batch size and position; freedom from side effects; per-window
failure; refusals; the host form."""
import ctypes as C

import numpy as np
import pytest

import dogleg_ref as DR
import hv_ref
import step_ref
import test_dogleg_step as TD
import test_gn_step as TG
from test_covariance_gpu import _window

pytestmark = pytest.mark.gpu

GAUGES = TD.GAUGES
# |p^| against Delta on branches 1 and 2: ten times the 1e-12 the numpy definition itself is held to (test_identities_of_the_definition)
TOL_RADIUS = 1e-11


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def refs(cfg, ocfg):
    """name -> (window, mu, {gauge: (radii, [the definition at each radius])}): computed once, shared and left unchanged"""
    out = {}
    for name, (make, mu) in DR.CASES.items():
        w = make(cfg, ocfg)
        sy, per = None, {}
        for gauge in GAUGES:
            with TG._ref():
                rad, gn = DR.radii(ocfg, w, mu, gauge, sys_=sy)
            sy = gn["sys"]
            per[gauge] = (rad, [DR.window_dogleg(ocfg, w, x, mu, gauge, gn=gn) for x in rad])
        out[name] = (w, mu, per)
    return out


def _part(r, i):
    a, b = r.offsets[i], r.offsets[i + 1]
    out = [np.array([getattr(r, f)[i] for f in DR.SCALARS]), np.array([getattr(r, f)[i] for f in ("branch", "n_free", "status")]),
           r.state_step[i], r.lm_step[a:b]]
    if r.cauchy_state is not None:
        out += [r.cauchy_state[i], r.cauchy_lm[a:b]]
    return out


def _bitwise(x, y):
    assert len(x) == len(y)
    for a, b in zip(x, y):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


def _got(r, i, w, sy):
    a, b = r.offsets[i], r.offsets[i + 1]
    g = {k: float(getattr(r, k)[i]) for k in DR.SCALARS}
    g["delta"] = step_ref.columns(w, sy, r.state_step[i], r.lm_step[a:b])
    g["cauchy"] = step_ref.columns(w, sy, r.cauchy_state[i], r.cauchy_lm[a:b]) if r.cauchy_state is not None else None
    return g


@pytest.mark.parametrize("case", sorted(DR.CASES))
def test_parity_with_numpy_on_every_branch(ctx, refs, case):
    from cerberus_amd import api
    w, mu, per = refs[case]
    b = api.Batch(ctx, [w.twin() for _ in range(3)])
    for gauge in GAUGES:
        rad, ref = per[gauge]
        r = b.dogleg_step(np.array(rad), mu=mu, gauge=gauge, cauchy=True)
        gn = b.gauss_newton_step(mu=mu, gauge=gauge)
        sy = ref[0]["sys"]
        for i in range(3):
            assert r.status[i] == 0 and r.branch[i] == i == ref[i]["branch"], (case, gauge, i, r.status[i], r.branch[i])
            e = DR.errors(sy, _got(r, i, w, sy), ref[i])
            print("MEASURED %s gauge %s branch %d: %s" % (case, gauge, i, " ".join("%s %.1e (%.0e)" % (k, x, DR.TOL[k]) for k, x in e.items())))
            for k, x in e.items():
                assert x <= DR.TOL[k], (case, gauge, i, k, x, DR.TOL[k])
            a, z = r.offsets[i], r.offsets[i + 1]
            for ss, ls in ((r.state_step[i], r.lm_step[a:z]), (r.cauchy_state[i], r.cauchy_lm[a:z])):
                full = np.concatenate([ss, ls])
                held = np.ones(full.size, bool)
                held[sy["pos"]] = False
                assert not full[held].any()
                if gauge == "frame0":
                    assert not ss[:3].any()
            assert r.n_free[i] == ref[i]["n_free"] == gn.n_free[i]
            assert r.model_cost_change[i] > 0.0 and r.grad_dot_step[i] < 0.0
            assert r.gauss_newton_norm[i].tobytes() == gn.scaled_norm[i].tobytes()
            full = np.concatenate([r.state_step[i], r.lm_step[a:z]])
            assert abs(r.norm[i] - np.linalg.norm(full)) <= 1e-13 * r.norm[i]
        # branch 0: the Gauss-Newton step call's bits
        assert r.state_step[0].tobytes() == gn.state_step[0].tobytes() and r.lm_step[:r.offsets[1]].tobytes() == gn.lm_step[:r.offsets[1]].tobytes()
        assert r.step_norm[0].tobytes() == gn.scaled_norm[0].tobytes() and r.beta[0] == 1.0 and r.beta[1] == 0.0
        for i in (1, 2):
            e = abs(r.step_norm[i] - rad[i]) / rad[i]
            print("MEASURED %s gauge %s branch %d: | |p^| / Delta - 1 | %.1e (%.0e)" % (case, gauge, i, e, TOL_RADIUS))
            assert e <= TOL_RADIUS
        assert r.step_norm[1] == rad[1]
        # the Cauchy point is -alpha c whatever the branch; on branch 1 the step is its multiple
        _bitwise([r.cauchy_state[0], r.cauchy_state[0]], [r.cauchy_state[1], r.cauchy_state[2]])
    assert api.lib().vilo_last_dogleg_step_ms(ctx.h) > 0.0
    b.close()


@pytest.mark.parametrize("case", ["prior", "no_prior", "two_frames", "field"])
def test_model_cost_change_against_the_hessian_vector_call(ctx, refs, ocfg, case):
    """model_cost_change (bilinearity of H [S u | delta_gn]) against hessian_vector's record for v = delta on the same batch, within that
    call's bounds on g . v and v^T H v (hv_ref.tol_gv, TOL_VHV, each in its own measure)."""
    from cerberus_amd import api
    w, mu, per = refs[case]
    with TG._ref():
        sy = hv_ref.system(ocfg, w)
    b = api.Batch(ctx, [w.twin() for _ in range(3)])
    for gauge in GAUGES:
        r = b.dogleg_step(np.array(per[gauge][0]), mu=mu, gauge=gauge)
        hv = b.hessian_vector(r.state_step, r.lm_step, state=False, landmarks=False)
        for i in range(3):
            v = np.abs(hv_ref.columns(sy, r.state_step[i], r.lm_step[r.offsets[i]:r.offsets[i + 1]]))
            bound = hv_ref.tol_gv(False) * float((sy["aJ"].T @ np.abs(sy["r"])) @ v) + 0.5 * hv_ref.TOL_VHV * float(v @ hv_ref.bound(sy, v))
            d = abs(r.model_cost_change[i] - hv.model_cost_change[i])
            print("MEASURED %s gauge %s branch %d: model_cost_change %.9e, hessian_vector's %.9e: difference %.1e (bound %.1e); g . delta %.1e of it"
                  % (case, gauge, i, r.model_cost_change[i], hv.model_cost_change[i], d, bound, abs(r.grad_dot_step[i] - hv.g_dot_v[i])))
            assert hv.status[i] == 0 and d <= bound
    b.close()


def test_one_caller_driven_iteration_against_the_solver(ctx, ocfg):
    """dogleg_step(radius 1e4, mu 1e-8) -> trial_cost -> retract where the relative decrease exceeds 1e-3, against one iteration of
    vilo_batch_solve on a fresh batch of the same windows and against the oracle's first iteration: the suite's 1e-8 state bound."""
    from cerberus_amd import api
    from oracle import oracle_py as O
    import test_branches as TB
    from cerberus_amd import synth
    cfg = synth.default_config()
    kws = (dict(seed=11), dict(seed=20, sig_p=0.2, sig_theta=0.08, sig_lambda_rel=0.6, sig_v=0.5), dict(seed=12, L=60))
    mine, theirs, orc = ([TB._window(cfg, ocfg, **kw) for kw in kws] for _ in range(3))
    a = api.Batch(ctx, mine)
    r = a.dogleg_step(1e4, mu=1e-8)
    assert (r.status == 0).all()
    t = a.trial_cost(r.state_step, r.lm_step)
    rel = t.cost_change / r.model_cost_change
    take = rel > 1e-3
    assert a.retract(r.state_step, r.lm_step, alpha=take.astype(float)).status.tolist() == [0] * len(kws)
    a.download()
    b = api.Batch(ctx, theirs)
    o = api.default_solve_opts(True, 1)
    o.initial_trust_region_radius = 1e4
    b.solve(o)
    summ = b.download()
    O.lib().orc_set_initial_mu.argtypes = [C.c_double]
    O.lib().orc_set_initial_mu(1e-8)
    for i, w in enumerate(orc):
        oo = O.default_opts(True, 1)
        oo.initial_trust_region_radius = 1e4
        osum = O.solve_window(ocfg, w, oo, check=False)
        sc = (C.c_double * 12)()
        O.lib().orc_last_step_scalars(sc)
        assert summ[i].num_successful == osum.num_successful == int(take[i]), (i, summ[i].num_successful, osum.num_successful, take[i])
        assert int(sc[10]) == r.branch[i]
        d_s, d_o = TG.state_distance(mine[i], theirs[i]), TG.state_distance(mine[i], w)
        e = TD.tie_errors({k: getattr(r, k)[i] for k in DR.SCALARS}, sc)
        e["cand"], e["rel"] = abs(t.cost[i] - sc[4]) / abs(sc[4]), abs(rel[i] - sc[5]) / abs(sc[5])
        print("MEASURED iteration %d (branch %d, taken %d): state against the solver's %.1e, against the oracle's %.1e; %s"
              % (i, r.branch[i], take[i], d_s, d_o, " ".join("%s %.1e" % kv for kv in e.items())))
        assert d_s <= 1e-8 and d_o <= 1e-8
        assert max(e.values()) <= DR.TIE_BOUND
    assert take.any()


def test_tie_to_the_oracles_trajectory(ctx, cfg, ocfg):
    """The device's dogleg at every state of the oracle's trajectories (tests/test_dogleg_step.py's, teacher forcing), at the oracle's radius
    and mu, against the oracle's scalars and branch: dogleg_ref.TIE_BOUND, ten times what the numpy definition measured on the CPU."""
    pts = [p for wkw, radius0, n in TD.TRAJECTORIES for p in TD.oracle_trajectory(cfg, ocfg, wkw, radius0, n)]
    r = ctx.window_dogleg_step([p[0] for p in pts], np.array([p[1] for p in pts]), mu=np.array([p[2] for p in pts]))
    worst = 0.0
    for i, (_, radius, mu, sc) in enumerate(pts):
        assert r.status[i] == 0 and r.branch[i] == int(sc[10]), (i, r.branch[i], sc[10])
        e = TD.tie_errors({k: getattr(r, k)[i] for k in DR.SCALARS}, sc)
        worst = max(worst, max(e.values()))
        print("MEASURED tie %d (radius %.3g mu %.1e branch %d): %s" % (i, radius, mu, r.branch[i], " ".join("%s %.1e" % kv for kv in e.items())))
    print("MEASURED tie: worst %.2e (bound %.0e)" % (worst, DR.TIE_BOUND))
    assert set(r.branch.tolist()) == {0, 1, 2} and worst <= DR.TIE_BOUND


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg, refs):
    from cerberus_amd import api
    w, mu, per = refs["prior"]
    other = _window(cfg, ocfg, seed=1302, L=50)
    for gauge, k in (("none", 2), ("frame0", 1), ("none", 0)):
        radius = per[gauge][0][k]
        alone = _part(api.Batch(ctx, [w.twin()]).dogleg_step(radius, mu=mu, gauge=gauge, cauchy=True), 0)
        assert alone[1][0] == k
        for n, positions in ((33, (0, 31, 32)), (257, (100,))):
            many = [other.twin() for _ in range(n)]
            for p in positions:
                many[p] = w.twin()
            rad = np.full(n, 3.0 * radius)
            rad[list(positions)] = radius
            b = api.Batch(ctx, many)
            r = b.dogleg_step(rad, mu=mu, gauge=gauge, cauchy=True)
            for p in positions:
                _bitwise(_part(r, p), alone)
            b.close()


def test_no_side_effects(ctx, cfg, ocfg):
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s, L=60) for s in (1311, 1312)]
    opts = api.default_solve_opts(True, 3)

    def sequence(report):
        ws = [w.twin() for w in base]
        b = api.Batch(ctx, ws)
        b.solve(opts)
        b.download()
        if report:
            before = [s.copy() for w in ws for s in w.state_arrays()]
            b.dogleg_step(1e4, mu=1e-8)
            bytes0 = b.device_bytes()
            for gauge in GAUGES:
                b.dogleg_step(np.array([1e-3, 1e4]), mu=1e-8, gauge=gauge, cauchy=True)
            assert b.device_bytes() == bytes0
            b.download()
            for x, y in zip(before, [s.copy() for w in ws for s in w.state_arrays()]):
                np.testing.assert_array_equal(x, y)
        b.solve(opts)
        summ = b.download()
        return [s.copy() for w in ws for s in w.state_arrays()], [bytes(s) for s in summ]
    st_a, su_a = sequence(False)
    st_b, su_b = sequence(True)
    for x, y in zip(st_a, st_b):
        np.testing.assert_array_equal(x, y)
    assert su_a == su_b


def test_failure_is_per_window(ctx, cfg, ocfg):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    good = _window(cfg, ocfg, seed=1321, L=40)
    alone = _part(api.Batch(ctx, [good.twin()]).dogleg_step(1.0, mu=1e-8), 0)
    n = 7
    ws = [good.twin() for _ in range(n)]
    ws[5].speed_bias[4, 1] = np.nan
    b = api.Batch(ctx, ws)
    mu = np.array([1e-8, np.nan, 1e-8, 1e-8, 1e-8, 1e-8, -1.0])
    rad = np.array([1.0, 1.0, 0.0, np.nan, 1.0, 1.0, 1.0])
    o, _, _ = api.dogleg_step_args(n, 1.0)
    rec, ss, ls = (T.WindowDoglegRecord * n)(), np.zeros((n, 222)), np.zeros(n * 40)
    p = lambda x: x.ctypes.data_as(T.c_double_p)
    assert api.lib().vilo_batch_dogleg_step(ctx.h, b.handle, C.byref(o), p(rad), p(mu), rec, p(ss), p(ls), None, None) == 0
    assert [rec[i].status for i in range(n)] == [0, 1, 1, 1, 0, 1, 1]
    for i in (1, 2, 3, 5, 6):
        assert np.isnan(ss[i]).all() and np.isnan(ls[40 * i:40 * i + 40]).all() and rec[i].branch == -1
        assert all(np.isnan(getattr(rec[i], f)) for f in DR.SCALARS)
    for i in (0, 4):
        assert ss[i].tobytes() == alone[2].tobytes() and ls[40 * i:40 * i + 40].tobytes() == alone[3].tobytes()
        assert [getattr(rec[i], f) for f in DR.SCALARS] == list(alone[0]) and rec[i].branch == alone[1][0]
    # an invalid window (a record without sqrt_info): status 2
    bad = good.twin()
    bad.preint = bad.preint.copy()
    bad.preint[2][33 + 961] = -1.0
    r = api.Batch(ctx, [good.twin(), bad]).dogleg_step(1.0, mu=1e-8, cauchy=True)
    assert list(r.status) == [0, 2] and np.isnan(r.state_step[1]).all() and np.isnan(r.lm_step[40:]).all() and np.isnan(r.cauchy_state[1]).all()
    _bitwise(_part(r, 0)[:4], alone)


def test_host_window_form_matches_batch(ctx, cfg, ocfg):
    from cerberus_amd import api
    ws = [_window(cfg, ocfg, seed=s, L=50) for s in (1331, 1332, 1333)]
    mu, rad = np.array([0.0, 1e-8, 1.0]), np.array([1e-2, 1e2, 1e6])
    for gauge in GAUGES:
        r = api.Batch(ctx, [w.twin() for w in ws]).dogleg_step(rad, mu=mu, gauge=gauge, cauchy=True)
        h = ctx.window_dogleg_step(ws, rad, mu=mu, gauge=gauge, cauchy=True)
        for i in range(3):
            _bitwise(_part(h, i), _part(r, i))


def test_refusals(ctx, cfg, ocfg):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    w = _window(cfg, ocfg, seed=1341, L=40)
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_dogleg_step
    rec, rad = (T.WindowDoglegRecord * 1)(), (C.c_double * 1)(1.0)
    assert f(ctx.h, b.handle, None, rad, None, None, None, None, None, None) == -2
    assert f(ctx.h, b.handle, None, None, None, rec, None, None, None, None) == -2
    assert f(ctx.h, None, None, rad, None, rec, None, None, None, None) == -2
    for field, value in (("gauge", 7), ("pad0", 1), ("min_pivot", -1.0), ("max_lm_diagonal", float("inf"))):
        o, _, _ = api.dogleg_step_args(1, 1.0)
        setattr(o, field, value)
        assert f(ctx.h, b.handle, C.byref(o), rad, None, rec, None, None, None, None) == -2
    assert f(ctx.h, b.handle, None, rad, None, rec, None, None, None, None) == 0 and rec[0].status == 0 and rec[0].n_free == 11 * 19 + 12 + 40
    mask = np.zeros(40, np.uint8)
    mask[3] = 1
    b.mask_landmarks(mask=mask)
    ss = np.full((1, 222), 7.0)
    rec[0].status, rec[0].alpha = 9, 7.0
    assert f(ctx.h, b.handle, None, rad, None, rec, ss.ctypes.data_as(T.c_double_p), None, None, None) == -5
    assert (ss == 7.0).all() and rec[0].status == 9 and rec[0].alpha == 7.0
    with pytest.raises(api.ViloError):
        b.dogleg_step(1.0)
    b.clear_mask()
    assert b.dogleg_step(1.0).status[0] == 0
