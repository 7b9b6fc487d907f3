"""GPU (-m gpu): vilo_batch_hessian_vector / vilo_window_hessian_vector against the numpy definition (tests/hv_ref.py) at hv_ref.TOL (the
product, componentwise against (|J|^T |J|) |v|), TOL_VHV and tol_gv(class) (the record) — ten times the FP64 floors tests/test_hess_vec.py
measures —, against gradient()'s diagonal, the tie to gauss_newton_step, symmetry on the device, bitwise independence of batch size,
position, K and k, the host form, NaN handling per vector, the mask's refusal and freedom from side effects."""
import ctypes as C

import numpy as np
import pytest

import const_windows as CW
import grad_ref
import hv_ref
import step_ref
import test_gn_step as TG
from test_covariance_gpu import _hip_free_bytes, _window
from test_gn_step_gpu import PERSISTENT, REINTEGRATED, _fetch

pytestmark = pytest.mark.gpu

NS = grad_ref.NS
CAP = 16
RECORD = ("vHv", "g_dot_v", "model_cost_change", "status")


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _pack(per_window):
    """[(state [K, 222], lm [K, L_w])] per window -> (state_vec [W, K, 222], lm_vec [K sum L]) of the call's layout"""
    return np.stack([s for s, _ in per_window]), np.concatenate([lm.ravel() for _, lm in per_window])


def _arrays(sy, w, dense):
    """dense vectors (dense_jacobian's column order) -> (state [K, 222], lm [K, L]); entries that are not read are NaN"""
    s, lm = np.full((len(dense), NS), np.nan), np.zeros((len(dense), w.L))
    for k, v in enumerate(dense):
        a, b = hv_ref.arrays(sy, v, w.L)
        free = np.zeros(NS + w.L, bool)
        free[sy["pos"]] = True
        s[k, free[:NS]], lm[k] = a[free[:NS]], b
    return s, lm


def _part(r, i, k=None):
    """the outputs of window i (vector k, or all) of a call with [W, K, 222] outputs"""
    from cerberus_amd import api
    lm = api.hess_vec_lm_block(r.lm_out, r.offsets, r.n_vec, i)
    sel = slice(None) if k is None else k
    return [r.state_out[i][sel], lm[sel], np.array([getattr(r, f)[i][sel] for f in RECORD[:3]]), np.array(r.status[i][sel])]


def _bitwise(x, y):
    for a, b in zip(x, y):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()


def _system(ocfg, w):
    with TG._ref():
        return hv_ref.system(ocfg, w)


def _check(r, i, w, sy, dense, tag, solved=False):
    """vectors 0 .. len(dense) - 1 of window i against the definition"""
    from cerberus_amd import api
    lm = api.hess_vec_lm_block(r.lm_out, r.offsets, r.n_vec, i)
    held = np.ones(NS + w.L, bool)
    held[sy["pos"]] = False
    worst = np.zeros(3)
    for k, v in enumerate(dense):
        assert r.status[i][k] == 0, (tag, k, r.status[i][k])
        full = np.concatenate([r.state_out[i][k], lm[k]])
        assert not full[held].any(), (tag, k)
        e = hv_ref.error(sy, full[sy["pos"]], v)
        e_v, e_g = hv_ref.scalar_errors(sy, v, r.vHv[i][k], r.g_dot_v[i][k])
        worst = np.maximum(worst, (e, e_v, e_g))
        assert r.model_cost_change[i][k] == -r.g_dot_v[i][k] - 0.5 * r.vHv[i][k], (tag, k)
    print("MEASURED %s: product %.1e (tolerance %.0e), vHv %.1e (%.0e), g.v %.1e (%.0e)"
          % (tag, worst[0], hv_ref.TOL, worst[1], hv_ref.TOL_VHV, worst[2], hv_ref.tol_gv(solved)))
    assert worst[0] <= hv_ref.TOL and worst[1] <= hv_ref.TOL_VHV and worst[2] <= hv_ref.tol_gv(solved), (tag, worst)


def _window_of(cfg, ocfg, name):
    if name == "prior_40":
        return _window(cfg, ocfg, seed=1201, L=40)
    if name == "no_prior_120":
        return _window(cfg, ocfg, seed=1202, L=120, prior=False)
    if name == "two_frames":
        return _window(cfg, ocfg, seed=1203, L=40, F=2, prior=False, leg_bias_const=1)
    if name == "five_frames":
        return _window(cfg, ocfg, seed=1204, L=40, F=5, prior=False, leg_bias_const=1)
    if name == "imu_only":
        return _window(cfg, ocfg, seed=1205, L=40, use_leg=0, leg_bias_const=1)
    if name == "prior_120_td_free":
        return _window(cfg, ocfg, seed=1206, L=120, td_const=0)
    return CW.leg_window(cfg, ocfg, "c40_ex_td")   # constant extrinsics, td free


@pytest.mark.parametrize("name", ["prior_40", "no_prior_120", "two_frames", "five_frames", "imu_only", "prior_120_td_free", "ex_const_td_free"])
def test_parity_with_numpy(ctx, cfg, ocfg, name):
    """Every test vector of hv_ref (seeded random in two scalings, -g, a unit vector per block kind, a landmark-only vector) in one call,
    the unread entries NaN; then K in {1, 3, 5, 16}: every column bitwise the column of the first call."""
    from cerberus_amd import api
    w = _window_of(cfg, ocfg, name)
    sy = _system(ocfg, w)
    dense = list(hv_ref.test_vectors(sy, 7).values())
    assert len(dense) <= CAP
    s, lm = _arrays(sy, w, dense)
    b = api.Batch(ctx, [w.twin()])
    r = b.hessian_vector(*_pack([(s, lm)]))
    _check(r, 0, w, sy, dense, name)
    for K in (1, 3, 5, CAP):
        idx = [(3 * K + j) % len(dense) for j in range(K)]
        rk = b.hessian_vector(*_pack([(s[idx], lm[idx])]))
        assert rk.n_vec == K and rk.state_out.shape == (1, K, NS)
        for j, k in enumerate(idx):
            _bitwise(_part(rk, 0, j), _part(r, 0, k))


@pytest.mark.parametrize("prior", [True, False])
def test_parity_at_a_solved_state(ctx, cfg, ocfg, prior):
    """Against the definition as at the initial state. hv_ref.tol_gv(solved) is a conditioning figure (g is a remainder of cancelling sums
    there) and does not hold the size of g_dot_v, so g_dot_v is also held against the gradient call's g on the same batch and state,
    whose g it is: two sums of n = 262 products in different orders differ by at most 2 n u |g|^T |v| = 6e-14 of it; held at the 1e-12
    of |g|^T |v| the tie to the step call holds grad_dot_step to."""
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=1291 + int(prior), L=40, prior=prior)
    b = api.Batch(ctx, [w])
    b.solve(api.default_solve_opts(True, 6))
    b.download()
    sy = _system(ocfg, w)
    dense = list(hv_ref.test_vectors(sy, 8).values())
    r = b.hessian_vector(*_pack([_arrays(sy, w, dense)]))
    _check(r, 0, w, sy, dense, "solved, prior %d" % prior, solved=True)
    g = b.gradient()
    gd = hv_ref.columns(sy, g.state_grad[0], g.lm_grad)
    worst = max(abs(r.g_dot_v[0][k] - float(gd @ v)) / float(np.abs(gd) @ np.abs(v)) for k, v in enumerate(dense))
    print("MEASURED solved, prior %d: g.v against the gradient call's g: %.1e of |g|.|v| (bound 1e-12)" % (prior, worst))
    assert worst <= 1e-12


def test_unit_vectors_give_the_gradient_calls_diagonal(ctx, cfg, ocfg):
    """(H e_i)_i against gradient().state_diag / lm_diag at that call's bound, grad_ref.TOL_H of h_i (both are held to it against the
    definition; the figure is printed), on 16 coordinates of every block kind and 16 landmarks."""
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=1211, L=120, td_const=0)
    b = api.Batch(ctx, [w])
    g = b.gradient()
    worst = 0.0
    state_idx = [0, 4, 35, 65, 66, 70, 74, 164, 165, 168, 208, 209, 214, 215, 220, 221]
    s = np.zeros((CAP, NS))
    s[np.arange(CAP), state_idx] = 1.0
    r = b.hessian_vector(s[None])
    for k, i in enumerate(state_idx):
        assert g.state_diag[0][i] > 0.0
        worst = max(worst, abs(r.state_out[0][k][i] - g.state_diag[0][i]) / g.state_diag[0][i])
        assert r.vHv[0][k] == r.state_out[0][k][i]
    lm_idx = [0, 1, 31, 32, 33, 63, 64, 65, 95, 96, 97, 100, 110, 117, 118, 119]
    lm = np.zeros((CAP, w.L))
    lm[np.arange(CAP), lm_idx] = 1.0
    r = b.hessian_vector(None, lm.ravel())
    for k, i in enumerate(lm_idx):
        worst = max(worst, abs(r.lm_out.reshape(CAP, w.L)[k][i] - g.lm_diag[i]) / g.lm_diag[i])
    print("MEASURED (H e_i)_i against the gradient call's diagonal: %.1e (tolerance %.0e)" % (worst, grad_ref.TOL_H))
    assert worst <= grad_ref.TOL_H


@pytest.mark.parametrize("prior,mu", [(True, 0.0), (True, 1e-8), (False, 1e-4)])
def test_tie_to_the_step_call(ctx, cfg, ocfg, prior, mu):
    """With delta from gauss_newton_step(mu): H delta + mu dd o delta + g, the residual of the system that call solves, as a componentwise
    backward error in the definition's system, at the bound of the case's class (step_ref.tol_eta). The record's model_cost_change,
    -g.delta - delta.H.delta / 2, against the step call's -g.delta / 2 + mu sum dd delta^2 / 2, at the bound tests/test_gn_step_gpu.py
    holds the step call's to: 1e-12 of |model_cost_change|. (The two differ by delta . residual / 2, so by at most the backward error
    times (|delta|^T |A| |delta| + |g|^T |delta|) / 2: that figure, several times wider, is printed beside it and not what is held.)"""
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=1221 + int(prior), L=40, prior=prior)
    b = api.Batch(ctx, [w])
    st = b.gauss_newton_step(mu=mu)
    assert st.status[0] == 0
    r = b.hessian_vector(st.state_step, st.lm_step)
    g = b.gradient()
    assert r.status[0] == 0
    with TG._ref():
        sy = step_ref.linear_system(ocfg, w)
    col = lambda s, lm: step_ref.columns(w, sy, s, lm)
    delta, y, gd = col(st.state_step[0], st.lm_step), col(r.state_out[0], r.lm_out), col(g.state_grad[0], g.lm_grad)
    A = np.abs(sy["H"]) + mu * np.diag(sy["dd"])
    den = A @ np.abs(delta) + np.abs(sy["g"])
    eta = float((np.abs(y + mu * sy["dd"] * delta + gd) / den).max())
    cls = step_ref.eta_class(False, prior, mu, "none")
    dm = abs(r.model_cost_change[0] - st.model_cost_change[0])
    dm_bound, dm_derived = 1e-12 * abs(st.model_cost_change[0]), step_ref.tol_eta(cls) * 0.5 * float(np.abs(delta) @ den)
    print("MEASURED tie to the step call, prior %d mu %g: backward error %.1e (class %s: tolerance %.0e); model_cost_change %.9e against the "
          "step call's %.9e: %.1e, %.1e of it (bound 1e-12 of it, %.1e; the backward error's own bound would be %.1e)"
          % (prior, mu, eta, cls, step_ref.tol_eta(cls), r.model_cost_change[0], st.model_cost_change[0], dm, dm / abs(st.model_cost_change[0]), dm_bound, dm_derived))
    assert eta <= step_ref.tol_eta(cls) and dm <= dm_bound
    assert abs(r.g_dot_v[0] - st.grad_dot_step[0]) <= 1e-12 * float(np.abs(gd) @ np.abs(delta))


def test_symmetry_on_the_device(ctx, cfg, ocfg):
    """u.(Hv) against v.(Hu) from one call of two vectors: each product is within TOL of the definition componentwise, so the two
    scalars differ by at most 2 TOL |u|^T |J|^T |J| |v| (and the definition's own two, 1e-14 of it: tests/test_hess_vec.py)."""
    from cerberus_amd import api
    w = _window(cfg, ocfg, seed=1231, L=120)
    sy = _system(ocfg, w)
    vs = hv_ref.test_vectors(sy, 9, unit=False)
    u, v = vs["random"], vs["random_plain"]
    r = api.Batch(ctx, [w]).hessian_vector(*_pack([_arrays(sy, w, [u, v])]))
    Hu, Hv = (np.concatenate([r.state_out[0][k], r.lm_out.reshape(2, w.L)[k]])[sy["pos"]] for k in (0, 1))
    d, den = abs(float(u @ Hv) - float(v @ Hu)), float(np.abs(u) @ hv_ref.bound(sy, v))
    print("MEASURED symmetry on the device: |u.Hv - v.Hu| = %.1e of |u|.|H||v| (bound %.0e)" % (d / den, 2 * hv_ref.TOL))
    assert d <= 2 * hv_ref.TOL * den


def _random_arrays(w, K, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(K, NS)), rng.normal(size=(K, w.L))


def test_independent_of_batch_size_position_and_column(ctx, cfg, ocfg):
    from cerberus_amd import api
    w, other = _window(cfg, ocfg, seed=1241, L=120), _window(cfg, ocfg, seed=1242, L=40)
    mine, theirs = _random_arrays(w, 5, 1), _random_arrays(other, 5, 2)
    alone = api.Batch(ctx, [w.twin()]).hessian_vector(*_pack([mine]))
    assert (alone.status == 0).all()
    # K and k: column 0 of the K = 5 call is the K = 1 call; a vector at column 15 of a full call, the others different
    one = api.Batch(ctx, [w.twin()]).hessian_vector(mine[0][:1][None], mine[1][0])
    _bitwise(_part(one, 0, 0), _part(alone, 0, 0))
    full = _random_arrays(w, CAP, 3)
    full[0][15], full[1][15] = mine[0][2], mine[1][2]
    _bitwise(_part(api.Batch(ctx, [w.twin()]).hessian_vector(*_pack([full])), 0, 15), _part(alone, 0, 2))
    # batch size and position
    eight = [other.twin() for _ in range(8)]
    eight[3] = w.twin()
    r = api.Batch(ctx, eight).hessian_vector(*_pack([mine if i == 3 else theirs for i in range(8)]))
    _bitwise(_part(r, 3), _part(alone, 0))
    at = (0, 150, 299)
    many = [w.twin() if i in at else other.twin() for i in range(300)]
    b = api.Batch(ctx, many)
    r = b.hessian_vector(*_pack([mine if i in at else theirs for i in range(300)]))
    for i in at:
        _bitwise(_part(r, i), _part(alone, 0))
    _bitwise(_part(r, 1), _part(r, 298))
    b.close()


def test_host_window_form_matches_batch(ctx, cfg, ocfg):
    from cerberus_amd import api
    ws = [_window(cfg, ocfg, seed=s, L=L) for s, L in ((1251, 50), (1252, 40), (1253, 70))]
    vec = _pack([_random_arrays(w, 3, 10 + i) for i, w in enumerate(ws)])
    r = api.Batch(ctx, [w.twin() for w in ws]).hessian_vector(*vec)
    h = ctx.window_hessian_vector(ws, *vec)
    for i in range(3):
        _bitwise(_part(h, i), _part(r, i))
    # one vector given as [W, 222]: [W, 222] and [W] come back, the same numbers
    r1 = api.Batch(ctx, [w.twin() for w in ws]).hessian_vector(vec[0][:, 0])
    r3 = api.Batch(ctx, [w.twin() for w in ws]).hessian_vector(vec[0][:, :1])
    assert r1.state_out.shape == (3, NS) and r1.vHv.shape == (3,) and r1.n_vec == 1
    assert r1.state_out.tobytes() == r3.state_out.tobytes() and r1.lm_out.tobytes() == r3.lm_out.tobytes() and r1.vHv.tobytes() == r3.vHv.tobytes()


def test_nan_is_per_vector_and_only_where_read(ctx, cfg, ocfg):
    from cerberus_amd import api
    # (a batch holds one IMU factor kind: the use_leg == 0 windows have a batch of their own)
    for wa, wb in ((_window(cfg, ocfg, seed=1261, L=40, F=5, prior=False, leg_bias_const=1, ex_const=1), _window(cfg, ocfg, seed=1264, L=50)),
                   (_window(cfg, ocfg, seed=1262, L=40, use_leg=0, leg_bias_const=1), _window(cfg, ocfg, seed=1265, L=50, use_leg=0, leg_bias_const=1))):
        va, vb = _random_arrays(wa, 3, 4), _random_arrays(wb, 3, 5)
        b = api.Batch(ctx, [wa.twin(), wb.twin()])
        ref = b.hessian_vector(*_pack([va, vb]))
        assert (ref.status == 0).all()
        for w, i in ((wa, 0), (wb, 1)):   # the outputs at entries that are not read are zero
            assert not ref.state_out[i][:, ~grad_ref.free_mask(w)].any() and ref.state_out[i][:, grad_ref.free_mask(w)].all()
        # NaN in every entry that is not read: absent frames, constant leg biases and extrinsics, td; the leg biases of a use_leg == 0 window
        na, nb = (va[0].copy(), va[1].copy()), (vb[0].copy(), vb[1].copy())
        na[0][:, ~grad_ref.free_mask(wa)] = np.nan
        nb[0][:, ~grad_ref.free_mask(wb)] = np.nan
        assert np.isnan(na[0][:, 165:209]).all() and np.isnan(nb[0][:, 221]).all()
        r = b.hessian_vector(*_pack([na, nb]))
        for i in (0, 1):
            _bitwise(_part(r, i), _part(ref, i))
        # NaN / inf in a read entry: that vector alone
        na[0][1, 7] = np.nan
        nb[1][2, 11] = np.inf
        r = b.hessian_vector(*_pack([na, nb]))
        assert r.status.tolist() == [[0, 1, 0], [0, 0, 1]]
        for w, i, k in ((wa, 0, 1), (wb, 1, 2)):   # (NaN where the vector is read; the entries that are not read stay zero)
            p, free = _part(r, i, k), grad_ref.free_mask(w)
            assert np.isnan(p[0][free]).all() and not p[0][~free].any() and np.isnan(p[1]).all() and np.isnan(p[2]).all()
        for i, k in ((0, 0), (0, 2), (1, 0), (1, 1)):
            _bitwise(_part(r, i, k), _part(ref, i, k))
    # an invalid window (a record without sqrt_info): status 2 for all of its vectors
    w2 = _window(cfg, ocfg, seed=1263, L=40)
    bad2 = w2.twin()
    bad2.preint = bad2.preint.copy()
    bad2.preint[2][33 + 961] = -1.0
    v2 = _random_arrays(w2, 3, 6)
    good = api.Batch(ctx, [w2.twin()]).hessian_vector(*_pack([v2]))
    r = api.Batch(ctx, [w2.twin(), bad2]).hessian_vector(*_pack([v2, v2]))
    assert r.status.tolist() == [[0, 0, 0], [2, 2, 2]] and np.isnan(r.state_out[1]).all() and np.isnan(_part(r, 1)[1]).all() and np.isnan(r.vHv[1]).all()
    _bitwise(_part(r, 0), _part(good, 0))


def test_refusals(ctx, cfg, ocfg):
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    w = _window(cfg, ocfg, seed=1271, L=40)
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_hessian_vector
    rec = (T.HessVecRecord * CAP)()
    s = np.ones((CAP, NS))
    p = s.ctypes.data_as(T.c_double_p)
    assert f(ctx.h, b.handle, 1, p, None, None, None, None) == -2
    assert f(ctx.h, None, 1, p, None, rec, None, None) == -2
    assert f(ctx.h, b.handle, 0, p, None, rec, None, None) == -2
    assert f(ctx.h, b.handle, CAP + 1, p, None, rec, None, None) == -2
    assert f(ctx.h, b.handle, CAP, p, None, rec, None, None) == 0 and rec[CAP - 1].status == 0 and rec[CAP - 1].vHv > 0.0
    assert f(ctx.h, b.handle, 2, None, None, rec, None, None) == 0 and rec[1].status == 0 and rec[1].vHv == 0.0   # (no vector: zero)
    assert api.lib().vilo_last_hess_vec_ms(ctx.h) > 0.0
    mask = np.zeros(40, np.uint8)
    mask[3] = 1
    b.mask_landmarks(mask=mask)
    assert f(ctx.h, b.handle, 1, p, None, rec, None, None) == -5
    with pytest.raises(api.ViloError, match="vilo_batch_hessian_vector"):
        b.hessian_vector(s[None, :1])
    b.clear_mask()
    assert b.hessian_vector(s[None, :1]).status[0, 0] == 0


@pytest.mark.parametrize("samples", [False, True])
def test_no_side_effects(ctx, cfg, ocfg, samples):
    """As tests/test_gn_step_gpu.py::test_no_side_effects: every persistent vilo_debug_fetch component is bytewise what it was, the states
    and summaries too, no device memory is kept, and the next solve is bitwise a fresh batch's."""
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s, L=60) for s in (1281, 1282)]
    vec = _pack([_random_arrays(w, 4, 20 + i) for i, w in enumerate(base)])
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
            assert (b.hessian_vector(*vec).status == 0).all()
            assert (b.hessian_vector(vec[0][:, 0]).status == 0).all()
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
                b.hessian_vector(*vec)
            assert b.device_bytes() == bytes0 and free0 - _hip_free_bytes() < (1 << 20)
        b.solve(opts)
        summ = b.download()
        return [s.copy() for w in ws for s in w.state_arrays()], [bytes(s) for s in summ]
    st_a, su_a = sequence(False)
    st_b, su_b = sequence(True)
    for x, y in zip(st_a, st_b):
        np.testing.assert_array_equal(x, y)
    assert su_a == su_b
