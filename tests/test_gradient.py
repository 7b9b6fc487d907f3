"""CPU: the gradient report's C-ABI (symbols, struct size, bad arguments without a device) and the definition the GPU pass is held to
(tests/grad_ref.py on ref_gradient.cost_and_gradient): against central differences of the oracle's window cost, the oracle's factor
classes against the compiled reference's, and the FP64 floor of the definition in the metric the GPU test uses
(err_i = |dg_i| / max(sqrt(h_i), |g_i|), |dh_i| / h_i). Measured floors (test_fp64_floor_measured prints them): see grad_ref.FLOOR_G / FLOOR_H."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import grad_ref
import resid_ref
from conftest import ROOT
from oracle import oracle_py as O
from oracle import ref_py as R
from test_covariance_gpu import _window


def test_symbols_exported():
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for n in ("vilo_batch_gradient", "vilo_window_gradient", "vilo_last_gradient_ms"):
        assert hasattr(lib, n), n


def test_python_binding_present():
    from cerberus_amd import api
    assert callable(getattr(api.Batch, "gradient", None))
    assert callable(getattr(api.Context, "window_gradient", None))


def test_struct_size_matches_header():
    from cerberus_amd import _ctypes as T
    assert C.sizeof(T.WindowGradient) == 48
    assert T.WindowGradient.argmax_kind.offset == 24 and T.WindowGradient.n_free.offset == 36 and T.WindowGradient.status.offset == 40
    assert "} vilo_window_gradient_record;" in open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    src = open(os.path.join(ROOT, "cerberus_amd", "csrc", "kernels_grad.hip")).read()
    assert "static_assert(sizeof(vilo_window_gradient_record) == 48" in src


def test_bad_arguments_without_a_device():
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    L = api.lib()
    wg = (T.WindowGradient * 1)()
    assert L.vilo_batch_gradient(None, None, wg, None, None, None, None) == -2
    assert L.vilo_window_gradient(None, 1, None, None, wg, None, None, None, None) == -2
    assert L.vilo_last_gradient_ms(None) == -1.0


# ---- the definition against central differences of the oracle's window cost ----
def _moved(w, pos, step):
    """a twin of w with local coordinate `pos` (0..221: state entry, 222 + l: inverse depth l) moved by `step`"""
    v = w.twin()
    if pos >= grad_ref.NS:
        v.inv_depth[pos - grad_ref.NS] += step
        return v
    arrs = {0: v.pose, 1: v.speed_bias, 2: v.leg_bias, 3: v.ex_pose, 4: v.td.reshape(1, 1)}
    for kind, first, size, n in grad_ref.BLOCKS:
        if first <= pos < first + size * n:
            i, c = (pos - first) // size, (pos - first) % size
            if kind in (0, 3):
                d = np.zeros(6)
                d[c] = step
                arrs[kind][i][:] = O.pose_plus(arrs[kind][i], d)
            else:
                arrs[kind][i][c] += step
    return v


def _parts(ocfg, w):
    """the window's cost part by part (tests/resid_ref.py): prior, IMU intervals, landmarks"""
    r = resid_ref.window_residuals(ocfg, w)
    return np.concatenate([[r["prior_cost"]], r["imu_cost"], r["lm_cost"]])


FD_CASES = [("prior", dict()), ("no_prior", dict(prior=False))]


@pytest.mark.parametrize("solved", [False, True])
@pytest.mark.parametrize("name,kw", FD_CASES)
def test_definition_against_central_differences(cfg, ocfg, name, kw, solved):
    """Steps as tests/test_oracle_factors.py takes them (1e-6 on poses, extrinsics, td and inverse depths, 1e-7 on speeds and biases; larger
    where the rounding of the cost itself asks for it, see below) and
    its tolerances, per entry in units of max(sqrt(h_i), |g_i|): 5e-3 for every entry an IMU factor or the prior touches (their Jacobians are
    the reference's first-order bias / rotation corrections, not the exact derivative: test_imu_factor_jacobians_fd's bound), 2e-5 for the
    entries only projection factors touch (test_projection_jacobians_fd's)."""
    w = _window(cfg, ocfg, seed=501 + len(name), L=16, **kw)
    if solved:
        O.solve_window(ocfg, w, O.default_opts(True, 8))
    cost, sg, sd, lg, ld, rec = grad_ref.window_gradient(ocfg, w)
    assert abs(cost - O.window_cost(ocfg, w)) <= 1e-13 * cost
    free = grad_ref.free_mask(w)
    g = np.concatenate([sg, lg])
    h = np.concatenate([sd, ld])
    prior = bool(w.prior.struct.valid)
    eps = np.finfo(float).eps
    worst = {5e-3: 0.0, 2e-5: 0.0}
    for pos in list(np.flatnonzero(free)) + [grad_ref.NS + l for l in range(w.L)]:
        tol = 5e-3 if (pos < 209 or (prior and pos < grad_ref.NS)) else 2e-5
        unit = max(np.sqrt(h[pos]), abs(g[pos]))
        step = 1e-7 if 66 <= pos < 209 else 1e-6
        cp, cm = _parts(ocfg, _moved(w, pos, step)), _parts(ocfg, _moved(w, pos, -step))
        # A difference of costs carries their rounding, eps * cost / step. The window's cost is differenced part by part (the parts the
        # entry does not touch cancel exactly), and where the parts it touches are large (an IMU interval at the initial state costs
        # ~1e12) the step grows until that rounding is 1 % of the tolerance.
        need = 100 * eps * float(np.abs(cp[cp != cm]).sum()) / (tol * unit)
        if need > step:
            step = need
            cp, cm = _parts(ocfg, _moved(w, pos, step)), _parts(ocfg, _moved(w, pos, -step))
        fd = math.fsum(cp - cm) / (2 * step)
        err = abs(fd - g[pos]) / unit
        worst[tol] = max(worst[tol], err)
        assert err <= tol, (pos, step, fd, g[pos], h[pos])
    print("MEASURED central differences, %s, solved %d: IMU / prior entries %.1e (5e-3), projection-only entries %.1e (2e-5)"
          % (name, solved, worst[5e-3], worst[2e-5]))
    assert rec["n_free"] == int(free.sum()) + w.L


@pytest.mark.skipif(not R.available(), reason="oracle/_ref/libref.so not built")
@pytest.mark.parametrize("name,kw", FD_CASES + [("td_free", dict(td_const=0)), ("imu_only", dict(use_leg=0, leg_bias_const=1))])
def test_oracle_classes_against_the_compiled_reference(cfg, ocfg, name, kw):
    w = _window(cfg, ocfg, seed=601 + len(name), L=60, **kw)
    O.solve_window(ocfg, w, O.default_opts(True, 6))
    a = grad_ref.window_gradient(ocfg, w)
    with R.as_oracle():
        b = grad_ref.window_gradient(ocfg, w)
    eg, eh = grad_ref.errors(w, a[1:5], b[1:5])
    print("MEASURED oracle against compiled reference, %s: gradient %.1e, diagonal %.1e" % (name, eg, eh))
    assert abs(a[0] - b[0]) <= 1e-12 * b[0]
    assert eg < 1e-3 and eh < 1e-3


def _ulp_moved(w, rng):
    v = w.twin()
    for a in v.state_arrays():
        a *= 1.0 + np.finfo(float).eps * rng.choice([-1.0, 1.0], size=a.shape)
    return v


def test_fp64_floor_measured(cfg, ocfg):
    """The spread of the definition in FP64: the same state with every entry moved by one unit in the last place (seeded signs), and the
    oracle's classes against the compiled reference's (where built), at the initial and at a solved state of windows with and without a
    prior. The GPU tolerances (grad_ref.TOL_G, TOL_H) are ten times grad_ref.FLOOR_G / FLOOR_H, which must stand above these figures."""
    rng = np.random.default_rng(7)
    fg, fh = 0.0, 0.0
    for name, kw in FD_CASES:
        for solved in (False, True):
            w = _window(cfg, ocfg, seed=701 + len(name), **kw)
            if solved:
                O.solve_window(ocfg, w, O.default_opts(True, 6))
            a = grad_ref.window_gradient(ocfg, w)[1:5]
            ug, uh = grad_ref.errors(w, grad_ref.window_gradient(ocfg, _ulp_moved(w, rng))[1:5], a)
            rg, rh = 0.0, 0.0
            if R.available():
                with R.as_oracle():
                    rg, rh = grad_ref.errors(w, a, grad_ref.window_gradient(ocfg, w)[1:5])
            print("MEASURED floor, %-8s solved %d: one ulp gradient %.1e diagonal %.1e; oracle against reference gradient %.1e diagonal %.1e"
                  % (name, solved, ug, uh, rg, rh))
            fg, fh = max(fg, ug, rg), max(fh, uh, rh)
    print("MEASURED floor: gradient %.1e, diagonal %.1e (grad_ref: FLOOR_G %.1e FLOOR_H %.1e, tolerances %.1e %.1e)"
          % (fg, fh, grad_ref.FLOOR_G, grad_ref.FLOOR_H, grad_ref.TOL_G, grad_ref.TOL_H))
    assert np.isfinite(fg) and np.isfinite(fh) and fg < 1e-3 and fh < 1e-3
