"""CPU: the numpy restatement of vilo_batch_retract (tests/retract_ref.py) against the oracle's local parameterisation, the argument checks
of api.retract_opts, the declarations, and the directional-derivative numbers of tests/test_retract_gpu.py produced by the oracle alone:
the oracle's cost along a unit direction, centrally differenced at retract_ref.EPS, against numpy's gradient."""
import ctypes as C
import os

import numpy as np
import pytest

import grad_ref
import retract_ref as RR
from conftest import ROOT, rand_pose


def _oracle_plus(X, S):
    from oracle import oracle_py as O
    return np.array([O.pose_plus(X[i], S[i]) for i in range(len(X))])


def test_numpy_pose_plus_against_the_oracle():
    """retract_ref.pose_plus_np and the oracle's Plus on random poses and steps. Measured: 2.2e-16, 3.3e-16, 2.2e-16 at step sizes 1e-2,
    1e-1, 1 (RR.PLUS_MEASURED = 3.4e-16); the bound is ten times that."""
    rng = np.random.default_rng(2026)
    worst = 0.0
    for scale in (1e-2, 1e-1, 1.0):
        X = np.array([rand_pose(rng, 10.0) for _ in range(2000)])
        S = scale * rng.normal(size=(2000, 6))
        e = float(np.abs(RR.pose_plus_np(X, S) - _oracle_plus(X, S)).max())
        print("MEASURED pose_plus_np against the oracle, steps of %.0e: %.2e" % (scale, e))
        worst = max(worst, e)
    assert worst <= RR.PLUS_TOL, worst


def test_restatement_on_a_window(cfg, ocfg):
    """The restatement itself, with the oracle's Plus: additive blocks are x + alpha * step, constant blocks, absent frames and masked
    landmarks stay whatever the step holds there, a non-finite applied entry or alpha leaves everything."""
    w = RR.kind_window(cfg, ocfg, "f60_partial8")
    w.ex_const = 1
    rng = np.random.default_rng(5)
    mask = np.zeros(w.L, np.uint8)
    mask[::7] = 1
    s, sl = RR.random_step(w, rng, lm_mask=mask)
    assert np.isnan(s).sum() == 3 * 6 + 3 * 9 + 11 * 4 + 12 + 1 and np.isnan(sl).sum() == int(mask.sum())   # F = 8, leg biases, extrinsics and td constant
    before = w.clone_state()
    out, rec = RR.retract(w, s, sl, 0.5, _oracle_plus, lm_mask=mask)
    assert rec["status"] == RR.OK and rec["n_applied"] == 8 * 15 + w.L - int(mask.sum())
    assert all(np.isfinite(a).all() for a in out)
    np.testing.assert_array_equal(out[1][:8], before[1][:8] + 0.5 * s[66:66 + 72].reshape(8, 9))
    for i in (2, 3, 4):
        assert out[i].tobytes() == before[i].tobytes()
    assert out[0][8:].tobytes() == before[0][8:].tobytes() and out[1][8:].tobytes() == before[1][8:].tobytes()
    assert out[5][mask != 0].tobytes() == before[5][mask != 0].tobytes() and (out[5][mask == 0] != before[5][mask == 0]).all()
    np.testing.assert_allclose(out[0][:8], RR.pose_plus_np(before[0][:8], 0.5 * s[:48].reshape(8, 6)), rtol=0, atol=RR.PLUS_TOL)
    sv = 0.5 * np.concatenate([s[np.isfinite(s)], sl[np.isfinite(sl)]])
    assert rec["step_max"] == np.abs(sv).max() and abs(rec["step_norm"] - np.linalg.norm(sv)) <= 1e-15 * rec["step_norm"]
    for bad_s, bad_a in ((np.where(np.arange(RR.NS) == 70, np.inf, s), 0.5), (s, np.nan)):
        out, rec = RR.retract(w, bad_s, sl, bad_a, _oracle_plus, lm_mask=mask)
        assert rec == dict(status=RR.NUMERIC, n_applied=0, step_norm=0.0, step_max=0.0)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(out, before))


def test_retract_opts_checks_its_arguments():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    o, s, l, a = api.retract_opts(3, 10)
    assert (o.base, o.reserved, s, l, a) == (T.RETRACT_BASE["current"], 0, None, None, None)
    o, s, l, a = api.retract_opts(3, 10, "uploaded", np.zeros((3, 222), np.float32), list(range(10)), [1, 2, 3])
    assert o.base == T.RETRACT_BASE["uploaded"] == 1
    for arr, shape in ((s, (3, 222)), (l, (10,)), (a, (3,))):
        assert arr.dtype == np.float64 and arr.flags["C_CONTIGUOUS"] and arr.shape == shape
    with pytest.raises(ValueError, match="base"):
        api.retract_opts(3, 10, "initial")
    for bad in (np.zeros((3, 221)), np.zeros((2, 222)), np.zeros(3 * 222), np.zeros((3, 222, 1))):
        with pytest.raises(ValueError, match="state_step"):
            api.retract_opts(3, 10, state_step=bad)
    for bad in (np.zeros(9), np.zeros(11), np.zeros((10, 1))):
        with pytest.raises(ValueError, match="lm_step"):
            api.retract_opts(3, 10, lm_step=bad)
    for bad in (np.zeros(2), np.zeros(4), np.zeros((3, 1)), 1.0):
        with pytest.raises(ValueError, match="alpha"):
            api.retract_opts(3, 10, alpha=bad)


def test_declarations():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    assert C.sizeof(T.RetractOpts) == 8 and C.sizeof(T.WindowRetractRecord) == 24
    assert T.RETRACT_OK == 0 and T.RETRACT_NUMERIC == 1 and T.GRAD_STATE == RR.NS
    assert api.Retraction._fields == ("status", "n_applied", "step_norm", "step_max")
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    for name in ("vilo_batch_retract", "vilo_window_retract", "vilo_default_retract_opts", "vilo_last_retract_ms", "vilo_batch_set_state",
                 "vilo_batch_save_state", "vilo_batch_restore_state", "} vilo_retract_opts;", "} vilo_window_retract_record;",
                 "#define VILO_RETRACT_BASE_UPLOADED 1", "#define VILO_RETRACT_NUMERIC 1"):
        assert name in hdr, name
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    o = T.RetractOpts(7, 7)
    lib.vilo_default_retract_opts(C.byref(o))
    assert (o.base, o.reserved) == (0, 0)
    for m in ("retract", "set_state", "save_state", "restore_state"):
        assert callable(getattr(api.Batch, m))
    assert callable(api.Context.window_retract)


@pytest.mark.parametrize("name", RR.LEG_KINDS + (RR.IMU_KIND,))
def test_directional_derivative_with_the_oracle_alone(cfg, ocfg, name):
    """What tests/test_retract_gpu.py's layout test computes on the device, here with the oracle's cost and numpy's gradient: the central
    difference of the cost along a unit direction over the free coordinates against g . d, in units of |g|. RR.EPS sits where the
    difference is trustworthy: the error at EPS is within ten times RR.DD_MEASURED (the largest figure over the kinds, 2.6e-10 on
    c40_lb), and neither ten times EPS nor a tenth of it is an order of magnitude better on every kind (measured: RR.EPS's comment). Then
    the preconditioned step -g / h comes down in cost within 20 halvings of alpha (measured: 0, on g2 1)."""
    from oracle import oracle_py as O
    w = RR.kind_window(cfg, ocfg, name)
    cost, sg, sd, lg, ld, rec = grad_ref.window_gradient(ocfg, w)
    assert cost == pytest.approx(O.window_cost(ocfg, w), rel=1e-12)
    ds, dl = RR.unit_direction(w, np.random.default_rng(RR.DD_SEED))
    fs, fl = RR.applied(w)
    assert not ds[~fs].any() and abs((ds * ds).sum() + (dl * dl).sum() - 1.0) < 1e-14
    gd = float((sg * ds).sum() + (lg * dl).sum())

    def cost_after(step_s, step_l):
        def at(alpha):
            t = w.twin()
            t.set_state(RR.retract(w, step_s, step_l, alpha, _oracle_plus)[0])
            return O.window_cost(ocfg, t)
        return at

    errs = {e: RR.dd_error(RR.central_difference(cost_after(ds, dl), e), gd, rec["norm"]) for e in (10 * RR.EPS, RR.EPS, 0.1 * RR.EPS)}
    print("MEASURED %s: |dd - g.d| / |g| = %s (g.d %.3e, |g| %.3e; held %.1e)"
          % (name, ", ".join("%.1e at %.0e" % (v, k) for k, v in errs.items()), gd, rec["norm"], RR.DD_TOL))
    assert errs[RR.EPS] <= RR.DD_TOL
    assert abs(gd) > 1e3 * RR.DD_TOL * rec["norm"]   # the direction sees the gradient: the comparison is not between two zeros
    with np.errstate(divide="ignore", invalid="ignore"):
        ps, pl = np.where(fs & (sd > 0), -sg / sd, 0.0), np.where(ld > 0, -lg / ld, 0.0)
    at = cost_after(ps, pl)
    halvings = next((k for k in range(21) if at(0.5 ** k) < cost), None)
    print("MEASURED %s: preconditioned step accepted after %s halvings" % (name, halvings))
    assert halvings is not None and halvings <= 20
