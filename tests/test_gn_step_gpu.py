"""GPU (-m gpu): vilo_batch_gauss_newton_step / vilo_window_gauss_newton_step against the numpy definition (tests/step_ref.py) at
step_ref.TOL (the step, in units of sqrt(h)) and step_ref.tol_eta(class) (componentwise backward error, one bound per class of case:
initial state, solved state, solved state without a prior under damping) — ten times the FP64 floors tests/test_gn_step.py measures; the
figure is printed beside ten times the numpy solve's backward error in its own system, which a device that forms H and g in another order
of the sums is not held to —, the tie to the oracle's first accepted Gauss-Newton iteration, the loop with retract / residuals /
gradient, bitwise independence of batch size and position, per-window failure, freedom from side effects, the host form and refusals."""
import ctypes as C

import numpy as np
import pytest

import grad_ref
import retract_ref as RR
import step_ref
import test_gn_step as TG
from test_covariance_gpu import CASES, _hip_free_bytes, _window
from test_landmark_covariance_gpu import _no_landmarks

pytestmark = pytest.mark.gpu

RECORD = ("model_cost_change", "scaled_norm", "norm", "grad_dot_step", "n_free", "status")
MUS = (0.0, 1e-8, 1.0)


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _part(r, i):
    a, b = r.offsets[i], r.offsets[i + 1]
    return [np.array([getattr(r, f)[i] for f in RECORD[:4]]), np.array([getattr(r, f)[i] for f in RECORD[4:]]), r.state_step[i], r.lm_step[a:b]]


def _bitwise(x, y):
    for a, b in zip(x, y):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


def _gauge(w, mu):
    """the gauge a case is run under: none where a prior or mu > 0 fixes the system, frame0 otherwise"""
    return "none" if (w.prior.struct.valid or mu > 0.0) else "frame0"


def _check(r, i, ocfg, w, mu, gauge, tag, sys_=None, solved=False):
    """window i of r against the definition at w's state arrays; returns the linear system for reuse"""
    with TG._ref():
        ref = step_ref.window_step(ocfg, w, mu, gauge, sys_=sys_)
    a, b = r.offsets[i], r.offsets[i + 1]
    if ref["status"] == 1:   # rank deficient by the definition's min_pivot (two frames, no prior, mu = 0): the device must say so too
        print("MEASURED %s mu %g gauge %s: status 1 by the definition, the device's %d" % (tag, mu, gauge, r.status[i]))
        assert r.status[i] == 1 and np.isnan(r.state_step[i]).all() and np.isnan(r.lm_step[a:b]).all() and np.isnan(r.norm[i]), tag
        return ref["sys"]
    assert ref["status"] == 0 and r.status[i] == 0, (tag, ref["status"], r.status[i])
    sy = ref["sys"]
    got = step_ref.columns(w, sy, r.state_step[i], r.lm_step[a:b])
    e, eta = step_ref.step_error(sy, got, ref["delta"]), step_ref.backward_error(w, sy, mu, gauge, got)
    cls = step_ref.eta_class(solved, bool(w.prior.struct.valid), mu, gauge)
    print("MEASURED %s mu %g gauge %s: step %.1e (tolerance %.0e), backward error %.1e (class %s: tolerance %.0e; ten times the numpy solve's own: %.0e)"
          % (tag, mu, gauge, e, step_ref.TOL, eta, cls, step_ref.tol_eta(cls), 10 * step_ref.ETA_OWN))
    assert e <= step_ref.TOL and eta <= step_ref.tol_eta(cls), (tag, mu, e, eta, cls)
    # structural zeros, the record from the downloaded arrays
    full = np.concatenate([r.state_step[i], r.lm_step[a:b]])
    held = np.ones(full.size, bool)
    held[sy["pos"]] = False
    assert not full[held].any(), tag
    assert r.n_free[i] == ref["n_free"], (tag, r.n_free[i], ref["n_free"])
    if gauge == "frame0":
        assert not r.state_step[i, :3].any()
    assert r.grad_dot_step[i] < 0.0 and r.model_cost_change[i] > 0.0, tag
    assert abs(r.norm[i] - np.linalg.norm(full)) <= 1e-13 * r.norm[i]
    m = -0.5 * r.grad_dot_step[i] + 0.5 * mu * r.scaled_norm[i] ** 2
    assert abs(r.model_cost_change[i] - m) <= 1e-12 * abs(m), tag
    return sy


def _run_all_mu(ctx, ocfg, w, tag):
    """every mu of MUS on a batch of one, then the three as a per-window array on a batch of three: bitwise the single calls"""
    from cerberus_amd import api
    b = api.Batch(ctx, [w.twin()])
    sy, single = None, []
    for mu in MUS:
        g = _gauge(w, mu)
        r = b.gauss_newton_step(mu=mu, gauge=g)
        sy = _check(r, 0, ocfg, w, mu, g, tag, sy)
        single.append(r)
    if w.prior.struct.valid:   # FRAME0 beside a prior: the rotation of the prior's rows and of the coupling
        for mu in MUS[:2]:
            _check(b.gauss_newton_step(mu=mu, gauge="frame0"), 0, ocfg, w, mu, "frame0", tag + " (prior, frame0)", sy)
    g = _gauge(w, MUS[0])
    b3 = api.Batch(ctx, [w.twin() for _ in MUS])
    r3 = b3.gauss_newton_step(mu=np.array(MUS), gauge=g)
    for i, mu in enumerate(MUS):
        if _gauge(w, mu) == g:
            _bitwise(_part(r3, i), _part(single[i], 0))
        else:
            _check(r3, i, ocfg, w, mu, g, tag + " (array)", sy)


@pytest.mark.parametrize("case", sorted(CASES))
def test_parity_with_numpy(ctx, cfg, ocfg, case):
    _run_all_mu(ctx, ocfg, _window(cfg, ocfg, seed=1101 + len(case), L=40 if len(case) % 2 else 120, **CASES[case]), case)


def _small(cfg, ocfg, name):
    import field_windows as FW
    import frame_windows as FRW
    if name == "two_frames":
        return _window(cfg, ocfg, seed=71, L=40, F=2, prior=False, leg_bias_const=1)
    if name == "no_landmarks":
        return _no_landmarks(_window(cfg, ocfg, seed=72, L=10))
    if name == "imu_only":
        return _window(cfg, ocfg, seed=73, L=40, use_leg=0, leg_bias_const=1)
    if name == "ex_const_td_free":
        return _window(cfg, ocfg, seed=74, L=40, ex_const=1, td_const=0)
    if name == "leg_bias_const_prior":
        return _window(cfg, ocfg, seed=75, L=40, leg_bias_const=1)
    if name == "field":
        return FW.field_window(cfg, ocfg, "f40")
    return FRW.leg_window(cfg, ocfg, "g5")


@pytest.mark.parametrize("name", ["two_frames", "no_landmarks", "imu_only", "ex_const_td_free", "leg_bias_const_prior", "field", "five_frames"])
def test_smallest_shapes(ctx, cfg, ocfg, name):
    _run_all_mu(ctx, ocfg, _small(cfg, ocfg, name), name)


@pytest.mark.parametrize("prior", [True, False])
def test_parity_at_a_solved_state(ctx, cfg, ocfg, prior):
    """The classes of case whose backward-error floor is not the initial state's: after a six-iteration solve, with a prior (none at mu 0
    and 1e-8, frame0 at mu 0), without one (frame0 at mu 0; none at mu 1e-4, where g is small against |A||z|)."""
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=91 + int(prior), L=40, prior=prior)
    b = api.Batch(ctx, [w])
    b.solve(api.default_solve_opts(True, 6))
    b.download()
    sy = None
    for gauge, mu in ((("none", 0.0), ("none", 1e-8), ("frame0", 0.0)) if prior else (("frame0", 0.0), ("none", 1e-4))):
        sy = _check(b.gauss_newton_step(mu=mu, gauge=gauge), 0, ocfg, w, mu, gauge, "solved, prior %d" % prior, sy, solved=True)


def test_resident_form(ctx, cfg, ocfg):
    """The form that keeps the coupling in LDS (one workgroup per CU; Context.set_gn_step_form) against the same definition at the same
    bounds, and against the streamed form to the step's tolerance (they split the landmark passes differently: rounding only)."""
    from cerberus_amd import api
    wp, wn = _window(cfg, ocfg, seed=95, L=120), _window(cfg, ocfg, seed=96, L=50, prior=False, F=6, leg_bias_const=1)
    b = api.Batch(ctx, [wp.twin(), wn.twin()])
    mu = np.array([1e-8, 0.0])
    ref = b.gauss_newton_step(mu=mu, gauge="frame0")
    ctx.set_gn_step_form("resident")
    try:
        r = b.gauss_newton_step(mu=mu, gauge="frame0")
        r_none = b.gauss_newton_step(mu=1e-8)
    finally:
        ctx.set_gn_step_form("streamed")
    for i, w in enumerate((wp, wn)):
        sy = _check(r, i, ocfg, w, mu[i], "frame0", "resident form %d" % i)
        _check(r_none, i, ocfg, w, 1e-8, "none", "resident form %d" % i, sy)
        assert step_ref.step_error(sy, step_ref.columns(w, sy, r.state_step[i], r.lm_step[r.offsets[i]:r.offsets[i + 1]]),
                                   step_ref.columns(w, sy, ref.state_step[i], ref.lm_step[r.offsets[i]:r.offsets[i + 1]])) <= step_ref.TOL
    assert api.lib().vilo_set_gn_step_form(ctx.h, 2) == -2


def test_tie_to_the_solver(ctx, ocfg):
    """retract(step(mu = 1e-8)) on a fresh batch against one solver iteration on another fresh batch of TG.tie_window, an accepted
    Gauss-Newton step; scaled_norm^2 and model_cost_change against the oracle's scalars. Bounds: ten times what the CPU test measured, the
    state's capped at 1e-8."""
    from cerberus_amd import api
    w_o = TG.tie_window(ocfg)
    sc, sm = TG.oracle_first_iteration(ocfg, w_o)
    assert int(sc[10]) == 0 and sm.num_successful == 1
    wa, wb = TG.tie_window(ocfg), TG.tie_window(ocfg)
    a = api.Batch(ctx, [wa])
    r = a.gauss_newton_step(mu=1e-8)
    assert r.status[0] == 0 and a.retract(r.state_step, r.lm_step).status[0] == 0
    a.download()
    b = api.Batch(ctx, [wb])
    o = api.default_solve_opts(True, 1)
    o.initial_trust_region_radius = TG.TIE_RADIUS
    b.solve(o)
    assert b.download()[0].num_successful == 1
    d_s, d_o = TG.state_distance(wa, wb), TG.state_distance(wa, w_o)
    e_n, e_m = abs(r.scaled_norm[0] ** 2 - sc[2]) / sc[2], abs(r.model_cost_change[0] - sc[3]) / abs(sc[3])
    print("MEASURED tie: stepped state against the device's one-iteration solve %.1e, against the oracle's %.1e; gnnorm2 %.1e, model %.1e"
          % (d_s, d_o, e_n, e_m))
    bound = min(10 * TG.TIE_STATE, 1e-8)
    assert d_s <= bound and d_o <= bound and e_n <= 10 * TG.TIE_GNNORM2 and e_m <= 10 * TG.TIE_MODEL


def test_cost_drops_by_the_model_and_slope_is_grad_dot_step(ctx, cfg, ocfg):
    """cost(x [+] delta) against cost(x) - model_cost_change to first order: the remainder beyond the quadratic model,
    |actual / model - 1|, is held to ten times the same figure of the numpy definition's step costed by the oracle on this window (plus
    1e-10 for the rounding of two costs eight orders apart), which a wrong factor in either term of model_cost_change (order one) cannot
    meet. And the slope of
    cost(x [+] alpha delta) at 0 from alpha in {0, 1e-3, 2e-3} (exact for a quadratic) against grad_dot_step in units of |g| |delta|:
    retract_ref.DD_TOL, the bound tests/test_retract_gpu.py holds g . d to."""
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=81, L=60)
    b = api.Batch(ctx, [w])
    r = b.gauss_newton_step(mu=1e-8)
    g = b.gradient(state=False, landmarks=False)
    b.save_state()
    c0 = float(b.residuals().cost[0])

    def at(alpha):
        b.restore_state()
        assert b.retract(r.state_step, r.lm_step, np.array([alpha])).status[0] == 0
        return float(b.residuals().cost[0])
    c1, ca, cb = at(1.0), at(1e-3), at(2e-3)
    from oracle import oracle_py as O
    import ref_gradient as RG
    v = w.twin()
    with TG._ref():
        ref = step_ref.window_step(ocfg, v, 1e-8, "none")
    c0r = O.window_cost(ocfg, v)
    RG.apply_step(v, ref["sys"]["cols"], ref["delta"])
    rem_ref = abs((c0r - O.window_cost(ocfg, v)) / ref["model_cost_change"] - 1.0)
    rem = abs((c0 - c1) / r.model_cost_change[0] - 1.0)
    slope = (4.0 * ca - 3.0 * c0 - cb) / 2e-3
    err = abs(slope - r.grad_dot_step[0]) / (g.norm[0] * r.norm[0])
    print("MEASURED loop: cost %.6e -> %.6e, model_cost_change %.6e (|actual / model - 1| %.1e, the definition's %.1e); slope %.9e against grad_dot_step %.9e: %.1e of |g||delta| (held %.1e)"
          % (c0, c1, r.model_cost_change[0], rem, rem_ref, slope, r.grad_dot_step[0], err, RR.DD_TOL))
    assert rem <= 10.0 * rem_ref + 1e-10
    assert err <= RR.DD_TOL


def test_caller_driven_iterations_reach_the_solvers_stationarity(ctx, cfg, ocfg):
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=82, L=60)
    a, b = api.Batch(ctx, [w.twin()]), api.Batch(ctx, [w.twin()])
    for _ in range(10):
        r = a.gauss_newton_step(mu=1e-8)
        assert r.status[0] == 0 and a.retract(r.state_step, r.lm_step).status[0] == 0
    b.solve(api.default_solve_opts(True, 10))
    mine, theirs = a.gradient(state=False, landmarks=False).scaled_max[0], b.gradient(state=False, landmarks=False).scaled_max[0]
    print("MEASURED scaled_max after ten caller-driven iterations %.1e, after a ten-iteration solve %.1e" % (mine, theirs))
    assert mine <= 10.0 * theirs


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg):
    from cerberus_amd import api
    w, other = _window(cfg, ocfg, seed=77, L=120), _window(cfg, ocfg, seed=78, L=120)
    alone = _part(api.Batch(ctx, [w.twin()]).gauss_newton_step(mu=1e-8), 0)
    eight = [other.twin() for _ in range(8)]
    eight[3] = w.twin()
    _bitwise(_part(api.Batch(ctx, eight).gauss_newton_step(mu=1e-8), 3), alone)
    for pos in (0, 150, 299):
        many = [other.twin() for _ in range(300)]
        many[pos] = w.twin()
        b = api.Batch(ctx, many)
        _bitwise(_part(b.gauss_newton_step(mu=1e-8), pos), alone)
        b.close()


def test_failure_is_per_window(ctx, cfg, ocfg):
    from cerberus_amd import api
    good, nop = _window(cfg, ocfg, seed=5, L=40), _window(cfg, ocfg, seed=6, L=40, prior=False)
    alone = _part(api.Batch(ctx, [good.twin()]).gauss_newton_step(), 0)
    b = api.Batch(ctx, [good.twin(), nop.twin(), good.twin(), good.twin(), good.twin()])
    mu = np.array([0.0, 0.0, 0.0, np.nan, 0.0])
    o, _ = api.gn_step_opts(5)
    n = 5
    from cerberus_amd import _ctypes as T
    rec, ss, ls = (T.WindowStepRecord * n)(), np.zeros((n, 222)), np.zeros(5 * 40)
    assert api.lib().vilo_batch_gauss_newton_step(ctx.h, b.handle, C.byref(o), mu.ctypes.data_as(T.c_double_p), rec, ss.ctypes.data_as(T.c_double_p),
                                                  ls.ctypes.data_as(T.c_double_p)) == 0
    assert [rec[i].status for i in range(n)] == [0, 1, 0, 1, 0]
    for i in (1, 3):
        assert np.isnan(ss[i]).all() and np.isnan(ls[40 * i:40 * i + 40]).all()
        assert all(np.isnan(getattr(rec[i], f)) for f in RECORD[:4])
    for i in (0, 2, 4):
        assert ss[i].tobytes() == alone[2].tobytes() and ls[40 * i:40 * i + 40].tobytes() == alone[3].tobytes()
        assert [getattr(rec[i], f) for f in RECORD[:4]] == list(alone[0])
    # an invalid window (a record without sqrt_info): status 2
    bad = good.twin()
    bad.preint = bad.preint.copy()
    bad.preint[2][33 + 961] = -1.0
    r = api.Batch(ctx, [good.twin(), bad]).gauss_newton_step()
    assert list(r.status) == [0, 2] and np.isnan(r.state_step[1]).all() and np.isnan(r.lm_step[40:]).all()
    _bitwise(_part(r, 0), alone)


# vilo_debug_fetch's components. PERSISTENT: what a batch keeps between calls — the solver's camera-side and landmark-side step vectors
# (4, 5, 6, 8, 9), the SolverState scalars with the cost trace and the phase clocks (10, 12), the landmark permutation (11), the records and
# the prepared records (13, 15), the records' form (17), the bias chain's hand-over buffers (18, 19, 20) — bytewise unchanged by the call.
# REINTEGRATED: with samples in force the call integrates the records again at the current state, in place, as the gradient call does.
# WORKSPACE, overwritten by the mode-0 linearisation by design and written again by the next solve before it reads them: the Gram slots
# (0), lm_E (1), lm_g of both buffers (2, 14), lm_w (3), the IMU linearisation (7). (16 is 13 of an IMU-only batch.)
PERSISTENT = (4, 5, 6, 8, 9, 10, 11, 12, 13, 15, 17, 18, 19, 20)
REINTEGRATED = (13, 15)
WORKSPACE = (0, 1, 2, 3, 7, 14)


def _fetch(b, what, win):
    return b.fetch(what, win).tobytes()


@pytest.mark.parametrize("samples", [False, True])
def test_no_side_effects(ctx, cfg, ocfg, samples):
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s, L=60) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)

    def sequence(report):
        ws = [w.twin() for w in base]
        b = api.Batch(ctx, ws)
        if samples:
            b.set_samples()
        b.solve(opts)
        summ0 = b.download()
        if report:
            before = [s.copy() for w in ws for s in w.state_arrays()]
            kept = PERSISTENT if not samples else tuple(k for k in PERSISTENT if k not in REINTEGRATED)
            fetched = {(k, i): _fetch(b, k, i) for k in kept for i in range(len(ws))}
            b.gauss_newton_step(mu=1e-8)
            b.gauss_newton_step(mu=0.0, gauge="frame0")
            changed = [(k, i) for (k, i), x in fetched.items() if _fetch(b, k, i) != x]
            assert not changed, changed
            summ1 = b.download()
            for x, y in zip(before, [s.copy() for w in ws for s in w.state_arrays()]):
                np.testing.assert_array_equal(x, y)
            for s0, s1 in zip(summ0, summ1):
                assert bytes(s0) == bytes(s1)
            free0 = _hip_free_bytes()
            bytes0 = b.device_bytes()
            for _ in range(5):
                b.gauss_newton_step(mu=1e-8)
            assert b.device_bytes() == bytes0 and free0 - _hip_free_bytes() < (1 << 20)
        b.solve(opts)
        summ = b.download()
        return [s.copy() for w in ws for s in w.state_arrays()], [bytes(s) for s in summ]
    st_a, su_a = sequence(False)
    st_b, su_b = sequence(True)
    for x, y in zip(st_a, st_b):
        np.testing.assert_array_equal(x, y)
    assert su_a == su_b


def test_host_window_form_matches_batch(ctx, cfg, ocfg):
    from cerberus_amd import api
    ws = [_window(cfg, ocfg, seed=s, L=50) for s in (21, 22, 23)]
    mu = np.array([0.0, 1e-8, 1.0])
    r = api.Batch(ctx, [w.twin() for w in ws]).gauss_newton_step(mu=mu)
    h = ctx.window_gauss_newton_step(ws, mu=mu)
    for i in range(3):
        _bitwise(_part(h, i), _part(r, i))


def test_refusals(ctx, cfg, ocfg):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    w = _window(cfg, ocfg, seed=3, L=40)
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_gauss_newton_step
    rec = (T.WindowStepRecord * 1)()
    assert f(ctx.h, b.handle, None, None, None, None, None) == -2
    assert f(ctx.h, None, None, None, rec, None, None) == -2
    o, _ = api.gn_step_opts(1)
    o.gauge = 7
    assert f(ctx.h, b.handle, C.byref(o), None, rec, None, None) == -2
    o, _ = api.gn_step_opts(1)
    o.min_pivot = -1.0
    assert f(ctx.h, b.handle, C.byref(o), None, rec, None, None) == -2
    assert f(ctx.h, b.handle, None, None, rec, None, None) == 0 and rec[0].status == 0 and rec[0].n_free == 11 * 19 + 12 + 40
    assert api.lib().vilo_last_gn_step_ms(ctx.h) > 0.0
    mask = np.zeros(40, np.uint8)
    mask[3] = 1
    b.mask_landmarks(mask=mask)
    assert f(ctx.h, b.handle, None, None, rec, None, None) == -5
    with pytest.raises(api.ViloError):
        b.gauss_newton_step()
    b.clear_mask()
    assert b.gauss_newton_step().status[0] == 0
