"""GPU (-m gpu): every call that reads vilo_config, at the alternative configuration of tests/alt_config.py (R_br a skew rotation, p_br
non-zero, rho_fix shifted, every noise value, g_norm, focal_length and huber_delta off their defaults), against the oracle built by
O.config_from of the same struct. At the default point a transposed R_br, a dropped p_br, `a` for `a * a` at huber_delta = 1.0 or a
literal left in a launch line give the same bits; here they do not (tests/test_alt_config.py holds that on a CPU, field by field).

Every bound is the one the default configuration's test of the same call applies; each test names it. tests/test_oracle_vs_reference.py
and tests/test_golden.py pin the oracle at this configuration to the reference's own sources.

phi_n and dphi_n have a case of their own. At 1e-5 they sit seven orders below the foot-velocity noise, and within the factors of
[0.5, 2] they move nothing the device computes from them by more than 4 bounds (tests/test_alt_config.py), so test_preintegrate_joint_noise
integrates at alt_config.joint_noise_config, where the two are 1e3 and 3e3 times their defaults and carry the covariance's entries."""
import numpy as np
import pytest

import alt_config as A
import field_windows as FW
import resid_ref
from oracle import oracle_py as O
from test_gpu_parity import _check_linearization, _check_marginalize, _force_samples, _fresh, _rel
from test_oracle_factors import _proj_setup

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def acfg(cfg):
    return A.alt_config(cfg)


@pytest.fixture(scope="module")
def oa(acfg):
    return O.config_from(acfg)


@pytest.fixture(scope="module")
def ctx(acfg):
    from cerberus_amd import api
    c = api.Context(acfg, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_force(acfg):
    """the same configuration with contact_sensor_type 2: foot forces instead of contact flags"""
    from cerberus_amd import api
    c = api.Context(A.with_type(acfg, 2), 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def awin(acfg, oa):
    """40-landmark window generated at the alternative configuration, records from the oracle at that configuration"""
    from cerberus_amd import synth
    w = synth.make_window(acfg, n_landmarks=40, seed=7)
    O.fill_preint(oa, w)
    return w


def _worst(name, **kv):
    print("MEASURED test_alt_config_gpu %s: " % name + ", ".join("%s %.2e" % (k, v) for k, v in kv.items()))


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_eval_proj(ctx, oa, kind):
    """test_gpu_parity.py::test_eval_proj (n = 97; residual rtol 1e-12 / atol 1e-11, Jacobian 1e-11): sqrt_info = focal_length / 1.5."""
    rng = np.random.default_rng(100 + kind)
    n = 97
    setups = [_proj_setup(rng, kind) for _ in range(n)]
    obs = np.stack([s[0] for s in setups])
    nb = len(setups[0][1])
    params = [np.stack([s[1][k] for s in setups]) for k in range(nb)]
    r, Js = ctx.eval_proj(kind, obs, params)
    er = ej = 0.0
    for i in range(n):
        r_o, J_o = O.eval_proj(kind, oa, obs[i], [p[i] for p in params])
        np.testing.assert_allclose(r[i], r_o, rtol=1e-12, atol=1e-11)
        er = max(er, float(np.abs(r[i] - r_o).max()))
        for k in range(nb):
            np.testing.assert_allclose(Js[k][i], J_o[k], rtol=1e-11, atol=1e-11 * max(1.0, np.abs(J_o[k]).max()), err_msg="kind %d block %d" % (kind, k))
            ej = max(ej, float(np.abs(Js[k][i] - J_o[k]).max() / max(1.0, np.abs(J_o[k]).max())))
    _worst("eval_proj[%d]" % kind, residual=er, jacobian=ej)


def test_eval_imu_leg_and_imu(ctx, oa, awin):
    """test_gpu_parity.py::test_eval_imu_leg_and_imu (residual 1e-11 per entry, Jacobian 1e-13 per row): g_norm in both factors."""
    w = awin
    P = [w.pose[:-1], w.speed_bias[:-1], w.leg_bias[:-1], w.pose[1:], w.speed_bias[1:], w.leg_bias[1:]]
    r, Js = ctx.eval_imu_leg(w.preint, P)
    er = ej = 0.0
    for k in range(10):
        r_o, J_o = O.eval_imu_leg(oa, w.preint[k], [p[k] for p in P])
        e = (np.abs(r[k] - r_o) / np.maximum(np.abs(r_o), 1e-12 * np.abs(r_o).max())).max()
        assert e < 1e-11, ("imu_leg residual", k, e)
        Jg, Jo = np.hstack([Js[b][k] for b in range(6)]), np.hstack(J_o)
        f = (np.linalg.norm(Jg - Jo, axis=1) / np.linalg.norm(Jo, axis=1)).max()
        assert f < 1e-13, ("imu_leg J", k, f)
        er, ej = max(er, e), max(ej, f)
    P4 = [w.pose[:-1], w.speed_bias[:-1], w.pose[1:], w.speed_bias[1:]]
    r, Js = ctx.eval_imu(w.preint_imu, P4)
    for k in range(10):
        r_o, J_o = O.eval_imu(oa, w.preint_imu[k], [p[k] for p in P4])
        e = (np.abs(r[k] - r_o) / np.maximum(np.abs(r_o), 1e-12 * np.abs(r_o).max())).max()
        assert e < 1e-11, ("imu residual", k, e)
        Jg, Jo = np.hstack([Js[b][k] for b in range(4)]), np.hstack(J_o)
        f = (np.linalg.norm(Jg - Jo, axis=1) / np.linalg.norm(Jo, axis=1)).max()
        assert f < 1e-13, ("imu J", k, f)
        er, ej = max(er, e), max(ej, f)
    _worst("eval_imu_leg_and_imu", residual=er, jacobian_rows=ej)


def _check_records(out, ocfg, smp, w, tag):
    """the device's ten records against the oracle's at test_gpu_parity.py::test_preintegrate's bounds"""
    ej = ec = ee = 0.0
    for k in range(10):
        a0, a1 = w.sample_offsets[k], w.sample_offsets[k + 1]
        a, b = out[k], O.preintegrate_imu_leg(ocfg, smp[a0:a1], w.lin[k])
        np.testing.assert_allclose(a[:33], b[:33], rtol=1e-12, atol=1e-14, err_msg="state k=%d" % k)
        assert _rel(a[33:33 + 961], b[33:33 + 961]) < 1e-11, ("jacobian", k)
        assert _rel(a[33 + 961:], b[33 + 961:]) < 1e-10, ("covariance", k, _rel(a[33 + 961:], b[33 + 961:]))
        ca, cb = a[33 + 961:], b[33 + 961:]
        big = np.abs(cb) > 1e-6 * np.abs(cb).max()
        assert np.abs(ca[big] / cb[big] - 1).max() < 1e-9
        ej, ec, ee = max(ej, _rel(a[33:33 + 961], b[33:33 + 961])), max(ec, _rel(ca, cb)), max(ee, float(np.abs(ca[big] / cb[big] - 1).max()))
    _worst(tag, jacobian=ej, covariance=ec, significant_entries=ee)


@pytest.mark.parametrize("ctype", [0, 2])
def test_preintegrate_joint_noise(cfg, acfg, awin, ctype):
    """phi_n and dphi_n (nd[18 .. 30) of the preintegration kernel) at alt_config.joint_noise_config, 1e3 and 3e3 times their defaults,
    both contact models: test_preintegrate's bounds against the oracle at the same struct. tests/test_alt_config.py holds that either
    field put back, or the two swapped, moves the significant covariance entries by 6e6 .. 3e9 of their 1e-9; here the records are also
    more than 1000 of that bound away from the alternative configuration's, whose joint noise is 1e-5."""
    from cerberus_amd import api
    w = awin
    jn = A.with_type(A.joint_noise_config(cfg), ctype)
    oj, oalt = O.config_from(jn), O.config_from(A.with_type(acfg, ctype))
    smp = _force_samples(w.samples, 3) if ctype == 2 else w.samples
    c = api.Context(jn, 0)
    try:
        out = c.preintegrate(smp, w.sample_offsets, w.lin)
    finally:
        c.close()
    _check_records(out, oj, smp, w, "preintegrate_joint_noise[type %d]" % ctype)
    for k in range(10):
        b = O.preintegrate_imu_leg(oalt, smp[w.sample_offsets[k]:w.sample_offsets[k + 1]], w.lin[k])
        ca, cb = out[k][33 + 961:], b[33 + 961:]
        big = np.abs(cb) > 1e-6 * np.abs(cb).max()
        assert np.abs(ca[big] / cb[big] - 1).max() > 1000 * 1e-9, k


@pytest.mark.parametrize("ctype", [0, 2])
def test_preintegrate(ctx, ctx_force, cfg, acfg, awin, ctype):
    """test_gpu_parity.py::test_preintegrate / test_preintegrate_contact_sensor_type_2 (state rtol 1e-12 / atol 1e-14, jacobian 1e-11 and
    covariance 1e-10 of the largest entry, significant covariance entries 1e-9), and each record more than 1e-3 relative away from the
    default configuration's in jacobian and covariance (the latter test's line 169)."""
    w = awin
    c = ctx_force if ctype == 2 else ctx
    o2, od = O.config_from(A.with_type(acfg, ctype)), O.config_from(A.with_type(cfg, ctype))
    smp = _force_samples(w.samples, 3) if ctype == 2 else w.samples
    out = c.preintegrate(smp, w.sample_offsets, w.lin)
    _check_records(out, o2, smp, w, "preintegrate[type %d]" % ctype)
    for k in range(10):
        a0, a1 = w.sample_offsets[k], w.sample_offsets[k + 1]
        a, ca = out[k], out[k][33 + 961:]
        d = O.preintegrate_imu_leg(od, smp[a0:a1], w.lin[k])
        assert _rel(a[33:33 + 961], d[33:33 + 961]) > 1e-3 and _rel(ca, d[33 + 961:]) > 1e-3, k
        assert _rel(a[11:23], d[11:23]) > 1e-3, k      # (delta_epsilon: R_br, p_br and rho_fix in the foot velocities)
    if ctype == 0:
        lin6 = np.ascontiguousarray(w.lin[:, :6])
        out_i = c.preintegrate_imu(w.samples, w.sample_offsets, lin6)
        for k in range(10):
            np.testing.assert_allclose(out_i[k][:17], w.preint_imu[k][:17], rtol=1e-12, atol=1e-14)
            assert _rel(out_i[k][17:], w.preint_imu[k][17:]) < 1e-10
            d = O.preintegrate_imu(od, w.samples[w.sample_offsets[k]:w.sample_offsets[k + 1]], lin6[k])
            assert _rel(out_i[k][17 + 225:], d[17 + 225:]) > 1e-3     # (an IMU-only record's jacobian reads no configuration value)


@pytest.mark.parametrize("imu_only", [False, True])
@pytest.mark.parametrize("force", [False, True])
def test_streaming_preintegration_equals_the_batch_bitwise(ctx, ctx_force, awin, force, imu_only):
    """test_gpu_parity.py::test_streaming_preintegration_equals_the_batch_bitwise's random-pieces driver on the push kernels of both
    kinds under both contact models: bitwise the batch call."""
    from cerberus_amd import api
    c = ctx_force if force else ctx
    w = awin
    smp = _force_samples(w.samples, 5) if force else w.samples
    lin = np.ascontiguousarray(w.lin[:, :6]) if imu_only else w.lin
    batch = c.preintegrate_imu(smp, w.sample_offsets, lin) if imu_only else c.preintegrate(smp, w.sample_offsets, lin)
    rng = np.random.default_rng(11)
    pool = api.PreintStreams(c, 16, imu_only=imu_only)
    try:
        ids = rng.permutation(16)[:10]
        pool.reset(ids, np.stack([smp[w.sample_offsets[k]] for k in range(10)]), lin)
        cursor = [int(w.sample_offsets[k]) + 1 for k in range(10)]
        while any(cursor[k] < w.sample_offsets[k + 1] for k in range(10)):
            sel, chunks = [], []
            for k in range(10):
                left = int(w.sample_offsets[k + 1]) - cursor[k]
                if left and rng.random() < 0.7:
                    n = int(rng.integers(1, min(left, 9) + 1))
                    sel.append(k); chunks.append(smp[cursor[k]:cursor[k] + n]); cursor[k] += n
            if not sel:
                continue
            off = np.concatenate([[0], np.cumsum([len(ch) for ch in chunks])])
            pool.push(ids[sel], np.concatenate(chunks), off)
        np.testing.assert_array_equal(pool.read(ids), batch)
    finally:
        pool.close()


def _states_err(wa, wb):
    return max(float(np.abs(a - b).max() / max(1.0, np.abs(b).max())) for a, b in zip(wa.state_arrays(), wb.state_arrays()) if a.size)


@pytest.mark.parametrize("ctype", [0, 2])
def test_whole_path_with_the_devices_own_preintegration(ctx, ctx_force, acfg, ctype):
    """test_gpu_parity.py::test_path_parity_with_the_oracles_own_preintegration (cost and states 1e-8): the device integrates the
    samples, whitens its own records and solves; the oracle does the same on its side. This is where acc_w, gyr_w, rho_c_n and rho_nc_n
    are seen: they move the covariance by less than its bound relative to its largest entry, and the whitened factors by 0.1 .. 0.7."""
    from cerberus_amd import api
    c = ctx_force if ctype == 2 else ctx
    o2 = O.config_from(A.with_type(acfg, ctype))

    def window():
        w = FW.field_window(acfg, o2, "f40")
        if ctype == 2:
            w.samples = _force_samples(w.samples, 3)
        return w
    w_g, w_o = window(), window()
    c.preintegrate_window(w_g)
    O.fill_preint(o2, w_o)
    sg = c.solve_windows([w_g], api.default_solve_opts(True, FW.ITERS))[0]
    so = O.solve_window(o2, w_o, O.default_opts(True, FW.ITERS))
    assert (sg.iterations, sg.num_successful) == (so.iterations, so.num_successful)
    np.testing.assert_allclose(sg.final_cost, so.final_cost, rtol=1e-8)
    e = _states_err(w_g, w_o)
    _worst("whole path[type %d]" % ctype, states=e, cost=abs(sg.final_cost / so.final_cost - 1))
    assert e < 1e-8, e


@pytest.mark.parametrize("ctype", [0, 2])
def test_solve_with_repropagation(ctx, ctx_force, acfg, ctype):
    """tests/test_repropagation.py: test_gpu_solve_with_repropagation_vs_oracle (initial cost 1e-9, final cost 1e-7, states 1e-8) and, for
    the force-based model, test_gpu_solve_with_repropagation_and_the_force_based_contact_model_vs_oracle (cost trace 1e-7, states 1e-7)."""
    from cerberus_amd import api, synth
    from test_oracle_vs_reference import force_samples
    c = ctx_force if ctype == 2 else ctx
    c2 = A.with_type(acfg, ctype)
    o2 = O.config_from(c2)
    iters = 5 if ctype == 2 else 6

    def window():
        w = synth.make_window(c2, params=synth.default_params(config=3, n_landmarks=40 if ctype == 0 else 60, seed=5 if ctype == 0 else 9))
        if ctype == 2:
            w.samples[...] = force_samples(w.samples, seed=4)
        O.fill_preint(o2, w)
        return w
    w_g, w_o = window(), window()
    b = api.Batch(c, [w_g])
    try:
        b.set_samples()
        b.solve(api.default_solve_opts(True, iters))
        sg = b.download()[0]
    finally:
        b.close()
    with O.repropagation(w_o):
        so = O.solve_window(o2, w_o, O.default_opts(True, iters))
    assert (sg.iterations, sg.num_successful) == (so.iterations, so.num_successful)
    np.testing.assert_allclose(sg.initial_cost, so.initial_cost, rtol=1e-9)
    if ctype == 2:
        np.testing.assert_allclose(list(sg.cost_trace[:iters + 1]), list(so.cost_trace[:iters + 1]), rtol=1e-7)
    np.testing.assert_allclose(sg.final_cost, so.final_cost, rtol=1e-7)
    e = _states_err(w_g, w_o)
    _worst("repropagation[type %d]" % ctype, states=e, cost=abs(sg.final_cost / so.final_cost - 1))
    assert e < (1e-7 if ctype == 2 else 1e-8), e


@pytest.mark.parametrize("name", ["f40", "f40_allmono"])
@pytest.mark.parametrize("consts", [(0, 0, 1), (1, 0, 0)])
def test_linearization_and_gauss_newton_step(ctx, acfg, oa, consts, name):
    """test_gpu_parity.py::test_linearization_and_gauss_newton_step through its helper _check_linearization (landmark blocks 1e-11,
    gradients 1e-10 / 1e-9, Gauss-Newton solution 1e-7, dogleg scalars 1e-7, cost 1e-10; landmark gradients 1e-9 on their own scale):
    focal_length and huber_delta in the visual rows, g_norm in the IMU rows."""
    gl_own = _check_linearization(ctx, oa, FW.field_window(acfg, oa, name), consts)
    _worst("linearization[%s, %s]" % (name, consts), landmark_gradients=gl_own)
    assert gl_own < 1e-9, gl_own


def test_residuals(ctx, acfg, oa, cfg):
    """tests/test_residuals_gpu.py::test_field_windows through its _check_parity, before and after a solve. n_huber_active and the other
    counts match exactly. The per-window cost is held to 1e-12 relative, that test's bound, not to the bit: it is a sum of a few hundred
    block costs which the kernel adds lane by lane and across waves and numpy adds landmark by landmark, and two orders of an FP64 sum of
    n terms differ by up to n ulp. 1e-12 is 4500 ulp, and a threshold of 1.0 for 0.6 moves the visual cost by 5e11 of it
    (tests/test_alt_config.py). lm_reproj_px (rtol 1e-12) reaches the kernel through the separate focal argument; residuals 1e-12 / 1e-11.
    The counts are not the ones a threshold of 1.0 gives."""
    from cerberus_amd import api
    from test_residuals_gpu import _check_parity, _obs_offsets
    ws, names = FW.batch_of(FW.field_set(acfg, oa, FW.BATCH_NAMES), len(FW.BATCH_NAMES))
    kw = dict(observations=True, imu=True)
    oo = _obs_offsets(ws)
    b = api.Batch(ctx, ws)
    try:
        r0 = b.residuals(**kw)
        refs0 = [resid_ref.window_residuals(oa, w) for w in ws]
        for i, ref in enumerate(refs0):
            _check_parity(r0, i, ref, oo)
            assert r0.n_huber_active[i] == ref["n_huber_active"] and r0.cost[i] == pytest.approx(ref["cost"], rel=1e-12)
            ob = ref["obs_residuals"]
            s2 = np.concatenate([(ob[:, 0:2] ** 2).sum(1), (ob[:, 2:4] ** 2).sum(1)])
            assert int((s2[~np.isnan(s2)] > cfg.huber_delta ** 2).sum()) != ref["n_huber_active"], names[i]
        b.solve(api.default_solve_opts(True, FW.ITERS))
        summ = b.download()
        r1 = b.residuals(**kw)
        for i, w in enumerate(ws):
            ref = resid_ref.window_residuals(oa, w)
            _check_parity(r1, i, ref, oo)
            assert abs(r0.cost[i] - summ[i].initial_cost) <= 1e-12 * abs(summ[i].initial_cost), names[i]
            assert abs(r1.cost[i] - summ[i].final_cost) <= 1e-12 * abs(summ[i].final_cost), names[i]
    finally:
        b.close()


def _two_windows(acfg, oa):
    from test_covariance_gpu import CASES, _window
    return {"f40": FW.field_window(acfg, oa, "f40"), "partial_F6": _window(acfg, oa, seed=411, **CASES["partial_F6"])}


@pytest.mark.parametrize("name", ["f40", "partial_F6"])
def test_gradient(ctx, acfg, oa, name):
    """tests/test_gradient_gpu.py::test_parity_with_numpy through its _check_parity (grad_ref.TOL_G, TOL_H), initial and solved;
    tests/ref_gradient.py takes the threshold from the configuration it is handed."""
    from cerberus_amd import api
    from test_gradient_gpu import _check_parity
    w = _two_windows(acfg, oa)[name]
    b = api.Batch(ctx, [w])
    try:
        _check_parity(b.gradient(), 0, oa, w, "alt " + name + " initial")
        b.solve(api.default_solve_opts(True, 6))
        b.download()
        _check_parity(b.gradient(), 0, oa, w, "alt " + name + " solved")
    finally:
        b.close()


@pytest.mark.parametrize("name", ["f40", "partial_F6"])
def test_covariance(ctx, acfg, oa, name):
    """tests/test_covariance_gpu.py::test_parity_with_numpy (cov_ref.tolerances, correlation-scaled), gauge frame0."""
    import cov_ref
    from test_covariance_gpu import _solved
    w = _two_windows(acfg, oa)[name]
    b = _solved(ctx, [w])
    try:
        fr, po, st = b.covariance(gauge="frame0", poses=True)
        assert st[0] == 0, (name, st)
        fr_r, po_r = cov_ref.window_covariance(oa, w, gauge="frame0")
        err = cov_ref.block_errors(fr[0], fr_r, po[0], po_r)
        tp, ts = cov_ref.tolerances(bool(w.prior.struct.valid))
        _worst("covariance[%s]" % name, **err)
        assert err["pose"] < tp and err["ex_td"] < tp and err["sb"] < ts, (name, err)
        assert np.all(fr[0][fr_r == 0.0] == 0.0) and np.all(po[0][po_r == 0.0] == 0.0), name
    finally:
        b.close()


@pytest.mark.parametrize("mode", [0, 1])
def test_marginalize(ctx, oa, awin, mode):
    """test_gpu_parity.py::test_marginalize through its _check_marginalize on the 40-landmark window: J0^T J0 and J0^T r0 1e-6 against
    O.marginalize, 2e-5 (MARGIN_OLD) / 1e-11 against the 60-digit Schur complement of the oracle's A.

    MARGIN_OLD leaves the helper's third reference out, the numpy Schur complement through an FP64 pseudo-inverse of the unequilibrated
    Amm, as test_marginalize_field_windows does where that reference does not resolve its own 1e-6 (tests/field_windows.py, MARG_NOTE):
    on this window cond(Amm) is 1.3e12 (3.6e11 at the default configuration), and with numpy and the oracle alone, on a CPU, the numpy
    Schur complement is 1.20e-6 of the largest entry from the 60-digit one while the oracle is 5.5e-8 from it. MARGIN_SECOND_NEW keeps it."""
    _check_marginalize(ctx, oa, awin, mode, "alt test_marginalize", pinv=(mode == 1))


def test_solve_parity(ctx, acfg, oa):
    """test_gpu_parity.py::test_solve_parity, four fixed iterations (equal decisions, cost and radius traces 1e-8, states 1e-8)."""
    from cerberus_amd import api
    iters = 4
    w_g, w_o = _fresh(acfg, oa, n_landmarks=40, seed=11), _fresh(acfg, oa, n_landmarks=40, seed=11)
    summ = ctx.solve_windows([w_g], api.default_solve_opts(True, iters))[0]
    osum = O.solve_window(oa, w_o, O.default_opts(True, iters))
    ct_g = np.array([summ.cost_trace[i] for i in range(iters + 1)]); ct_o = np.array([osum.cost_trace[i] for i in range(iters + 1)])
    rt_g = np.array([summ.radius_trace[i] for i in range(iters + 1)]); rt_o = np.array([osum.radius_trace[i] for i in range(iters + 1)])
    assert summ.iterations == osum.iterations and summ.num_successful == osum.num_successful
    np.testing.assert_allclose(ct_g, ct_o, rtol=1e-8)
    np.testing.assert_allclose(rt_g, rt_o, rtol=1e-8)
    e = _states_err(w_g, w_o)
    _worst("solve_parity[4]", states=e, cost=float(np.abs(ct_g / ct_o - 1).max()))
    assert e < 1e-8, e


def test_sliding_window_resident_and_host_paths(ctx, cfg, acfg):
    """tests/test_sliding_window.py::test_resident_prior_equals_the_host_carried_one's replay under the alternative configuration: the
    resident and the host-carried path give the same estimate bit for bit. Both go through the same host window manager, so this does
    NOT check the focal length that manager keeps (a literal there would give both sides the same bits); it checks that the two paths
    hand the device the same configuration. That the replay reads the configuration at all: the estimate is not the one the same stream
    gives under the default configuration."""
    from cerberus_amd import api
    from test_sliding_window import _run
    a = _run(ctx, acfg, 20, seed=41)
    b = _run(ctx, acfg, 20, seed=41, resident=0)
    cd = api.Context(cfg, 0)
    try:
        d = _run(cd, cfg, 20, seed=41)
    finally:
        cd.close()
    assert not np.array_equal(a[1][-1][1]["Ps"], d[1][-1][1]["Ps"])
    for (_, sa), (_, sb) in zip(a[1], b[1]):
        for key in ("Ps", "Rs", "Vs", "Bas", "Bgs", "Rho"):
            np.testing.assert_array_equal(sa[key], sb[key])
        assert sa["prior_n"] == sb["prior_n"]
