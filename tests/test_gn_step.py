"""CPU: the Gauss-Newton step call's C-ABI (symbols, struct sizes, option and mu validation without a device) and the definition the GPU
pass is held to (tests/step_ref.py): the dense solve against the kernel's elimination order, the FP64 floor of the definition (one-ulp-moved
states; the oracle's classes against the compiled reference's), the componentwise backward error, the tie to the oracle's first accepted
Gauss-Newton iteration, and the structural cases. Measured figures are printed; step_ref.FLOOR / ETA_OWN / ETA_FLOORS stand above them."""
import ctypes as C
import os

import numpy as np
import pytest

import ref_gradient as RG
import step_ref
from conftest import ROOT
from oracle import oracle_py as O
from oracle import ref_py as R
from test_covariance_gpu import _window


def _ref():
    """the compiled reference's Evaluate where libref.so exists, otherwise the oracle's classes"""
    import contextlib
    return R.as_oracle() if R.available() else contextlib.nullcontext()


def test_symbols_exported():
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for n in ("vilo_batch_gauss_newton_step", "vilo_window_gauss_newton_step", "vilo_last_gn_step_ms", "vilo_default_step_opts"):
        assert hasattr(lib, n), n


def test_python_binding_present():
    from cerberus_amd import api
    assert callable(getattr(api.Batch, "gauss_newton_step", None))
    assert callable(getattr(api.Context, "window_gauss_newton_step", None))
    assert api.GaussNewtonStep._fields == ("state_step", "lm_step", "offsets", "model_cost_change", "scaled_norm", "norm", "grad_dot_step",
                                           "n_free", "status")


def test_struct_sizes_match_header():
    from cerberus_amd import _ctypes as T
    assert C.sizeof(T.StepOpts) == 32 and C.sizeof(T.WindowStepRecord) == 40
    assert T.StepOpts.min_lm_diagonal.offset == 8 and T.StepOpts.min_pivot.offset == 24
    assert T.WindowStepRecord.n_free.offset == 32 and T.WindowStepRecord.status.offset == 36
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    assert "} vilo_step_opts;" in hdr and "} vilo_window_step_record;" in hdr
    src = open(os.path.join(ROOT, "cerberus_amd", "csrc", "kernels_step.hip")).read()
    assert "static_assert(sizeof(vilo_step_opts) == 32" in src and "static_assert(sizeof(vilo_window_step_record) == 40" in src


def test_defaults_and_bad_arguments_without_a_device():
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    L = api.lib()
    o = T.StepOpts()
    L.vilo_default_step_opts(C.byref(o))
    assert (o.gauge, o.pad0, o.min_lm_diagonal, o.max_lm_diagonal, o.min_pivot) == (T.COV_GAUGES["none"], 0, 1e-6, 1e32, 1e-14)
    rec = (T.WindowStepRecord * 1)()
    assert L.vilo_batch_gauss_newton_step(None, None, None, None, rec, None, None) == -2
    assert L.vilo_window_gauss_newton_step(None, 1, None, None, None, None, rec, None, None) == -2
    assert L.vilo_last_gn_step_ms(None) == -1.0


def test_gn_step_opts_validation():
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    o, mu = api.gn_step_opts(3)
    assert mu is None and o.gauge == T.COV_GAUGES["none"] and o.min_lm_diagonal == 1e-6 and o.max_lm_diagonal == 1e32
    o, mu = api.gn_step_opts(3, mu=1e-8, gauge="frame0")
    assert o.gauge == T.COV_GAUGES["frame0"] and mu.shape == (3,) and (mu == 1e-8).all() and mu.flags.c_contiguous
    assert api.gn_step_opts(2, mu=[0.0, 2.0])[1].tolist() == [0.0, 2.0]
    for bad in (dict(gauge="frame1"), dict(mu=[1.0, 2.0]), dict(mu=np.zeros((3, 1))), dict(mu=-1e-9), dict(mu=[0.0, np.nan, 0.0]),
                dict(mu=np.inf), dict(min_lm_diagonal=-1.0), dict(min_lm_diagonal=2.0, max_lm_diagonal=1.0), dict(max_lm_diagonal=np.inf),
                dict(min_pivot=-1e-3), dict(min_pivot=np.nan)):
        with pytest.raises(ValueError):
            api.gn_step_opts(3, **bad)


# ---- the definition ----
# (L, prior, gauge, mu) of the floor measurement
FLOOR_CASES = [(L, p, g, mu) for L in (40, 120) for p, g, mu in ((True, "none", 0.0), (True, "none", 1e-8), (False, "frame0", 0.0), (False, "none", 1e-4))]


def _ulp_moved(w, rng):
    v = w.twin()
    for a in v.state_arrays():
        a *= 1.0 + np.finfo(float).eps * rng.choice([-1.0, 1.0], size=a.shape)
    return v


def test_dense_and_eliminated_orders_agree(cfg, ocfg):
    worst = 0.0
    for L, prior, gauge, mu in FLOOR_CASES[:4]:
        w = _window(cfg, ocfg, seed=801 + L, L=L, prior=prior)
        with _ref():
            a = step_ref.window_step(ocfg, w, mu, gauge)
        b = step_ref.window_step(ocfg, w, mu, gauge, order="eliminated", sys_=a["sys"])
        assert a["status"] == 0 and b["status"] == 0
        e = step_ref.step_error(a["sys"], b["delta"], a["delta"])
        print("MEASURED dense against eliminated order, L %d prior %d gauge %s mu %g: %.1e" % (L, prior, gauge, mu, e))
        worst = max(worst, e)
    assert worst <= step_ref.FLOOR


def test_fp64_floor_measured(cfg, ocfg):
    """The spread of the definition in FP64, as DESIGN 4.16 measured the gradient's: every state entry moved by one unit in the last place
    (seeded signs), and the oracle's classes against the compiled reference's (where built), in the metric of the GPU test and as the
    componentwise backward error of the eliminated-order solve: in its own system (ETA_OWN), and of the moved problem's step in the
    unmoved system, per class of case (step_ref.ETA_FLOORS): a kernel that linearises the same state in another order of the sums cannot
    be held closer than its class's figure."""
    rng = np.random.default_rng(11)
    fl, self_eta = 0.0, 0.0
    fe = {c: 0.0 for c in step_ref.ETA_FLOORS}
    for L, prior, gauge, mu in FLOOR_CASES:
        for solved in (False, True):
            w = _window(cfg, ocfg, seed=901 + L + int(prior), L=L, prior=prior)
            if solved:
                O.solve_window(ocfg, w, O.default_opts(True, 6))
            with _ref():
                a = step_ref.window_step(ocfg, w, mu, gauge, order="eliminated")
                m = step_ref.window_step(ocfg, _ulp_moved(w, rng), mu, gauge, order="eliminated")
            o = step_ref.window_step(ocfg, w, mu, gauge, order="eliminated") if R.available() else a
            assert a["status"] == 0 and m["status"] == 0 and o["status"] == 0
            sy = a["sys"]
            e_u, e_o = step_ref.step_error(sy, m["delta"], a["delta"]), step_ref.step_error(sy, o["delta"], a["delta"])
            n_u, n_o = step_ref.backward_error(w, sy, mu, gauge, m["delta"]), step_ref.backward_error(w, sy, mu, gauge, o["delta"])
            n_s = step_ref.backward_error(w, sy, mu, gauge, a["delta"])
            print("MEASURED floor, L %3d prior %d gauge %-6s mu %-5g solved %d: step one ulp %.1e oracle/reference %.1e; backward error "
                  "own %.1e one ulp %.1e oracle/reference %.1e" % (L, prior, gauge, mu, solved, e_u, e_o, n_s, n_u, n_o))
            cls = step_ref.eta_class(solved, prior, mu, gauge)
            fl, fe[cls], self_eta = max(fl, e_u, e_o), max(fe[cls], n_u, n_o), max(self_eta, n_s)
    print("MEASURED floor: step %.1e (FLOOR %.0e, TOL %.0e); backward error in the solve's own system %.1e (ETA_OWN %.0e); per class %s (ETA_FLOORS %s)"
          % (fl, step_ref.FLOOR, step_ref.TOL, self_eta, step_ref.ETA_OWN, {c: "%.1e" % v for c, v in fe.items()}, step_ref.ETA_FLOORS))
    assert fl <= step_ref.FLOOR and self_eta <= step_ref.ETA_OWN
    for c, v in fe.items():
        assert v <= step_ref.ETA_FLOORS[c], (c, v)


# the window of the solver tie: seed 11 of tests/test_branches.py with a large radius, whose first iteration is an accepted Gauss-Newton step
TIE = dict(seed=11, L=40)
TIE_RADIUS = 1e16
# what test_tie_to_the_oracles_first_iteration measured (state, gnnorm2, model), rounded up; the GPU bounds are ten times these, the
# state's capped at the project's 1e-8
TIE_STATE, TIE_GNNORM2, TIE_MODEL = 5e-10, 2e-11, 1e-14   # measured 4.7e-10, 1.1e-11, 2.2e-15


def tie_window(ocfg):
    from cerberus_amd import synth
    w = synth.make_window(synth.default_config(), params=synth.default_params(n_landmarks=TIE["L"], seed=TIE["seed"], with_prior=True))
    O.fill_preint(ocfg, w)
    return w


def oracle_first_iteration(ocfg, w):
    """one oracle iteration on w (in place) at initial mu 1e-8 and TIE_RADIUS: (scalars, summary)"""
    O.lib().orc_set_initial_mu.argtypes = [C.c_double]
    O.lib().orc_set_initial_mu(1e-8)
    o1 = O.default_opts(True, 1)
    o1.initial_trust_region_radius = TIE_RADIUS
    sm = O.solve_window(ocfg, w, o1, check=False)
    sc = (C.c_double * 12)()
    O.lib().orc_last_step_scalars(sc)
    return list(sc), sm


def state_distance(a, b):
    return max(float(np.abs(x - y).max() / max(1.0, np.abs(y).max())) for x, y in zip(a.state_arrays(), b.state_arrays()) if x.size)


def test_tie_to_the_oracles_first_iteration(ocfg):
    w_o = tie_window(ocfg)
    sc, sm = oracle_first_iteration(ocfg, w_o)
    assert int(sc[10]) == 0 and sm.num_successful == 1, (sc[10], sm.num_successful)
    w = tie_window(ocfg)
    with _ref():
        st = step_ref.window_step(ocfg, w, 1e-8, "none")
    assert st["status"] == 0
    RG.apply_step(w, st["sys"]["cols"], st["delta"])
    d = state_distance(w, w_o)
    e_n, e_m = abs(st["scaled_norm"] ** 2 - sc[2]) / sc[2], abs(st["model_cost_change"] - sc[3]) / abs(sc[3])
    print("MEASURED tie to the oracle's first iteration: state %.1e, gnnorm2 %.1e, model_cost_change %.1e" % (d, e_n, e_m))
    assert d <= TIE_STATE and e_n <= TIE_GNNORM2 and e_m <= TIE_MODEL


def test_structural_cases(cfg, ocfg):
    import grad_ref
    # constant blocks, an absent-frame window and the gauge-held directions are exactly zero; g . delta < 0
    for kw, gauge, mu in ((dict(ex_const=1, leg_bias_const=1), "none", 0.0), (dict(F=6, prior=False, leg_bias_const=1), "frame0", 0.0),
                          (dict(prior=False), "frame0", 1e-8), (dict(use_leg=0, leg_bias_const=1), "none", 1e-8)):
        w = _window(cfg, ocfg, seed=31, L=40, **kw)
        st = step_ref.window_step(ocfg, w, mu, gauge)
        assert st["status"] == 0 and st["grad_dot_step"] < 0.0 and st["model_cost_change"] > 0.0, kw
        free = grad_ref.free_mask(w)
        assert not st["state_step"][~free].any()
        assert st["n_free"] == int(free.sum()) + w.L - (4 if gauge == "frame0" else 0)
        if gauge == "frame0":
            u = __import__("cov_ref").quat_R(w.pose[0, 3:7])[2]
            assert not st["state_step"][:3].any() and abs(u @ st["state_step"][3:6]) <= 1e-15 * np.abs(st["state_step"][3:6]).max()
    # mu -> infinity: delta -> -g / (mu D^2 / s^2)
    w = _window(cfg, ocfg, seed=32, L=40)
    st = step_ref.window_step(ocfg, w, 1e30, "none")
    lim = -st["sys"]["g"] / (1e30 * st["sys"]["dd"])
    assert st["status"] == 0 and np.abs(st["delta"] - lim).max() <= 1e-12 * np.abs(lim).max()
    # a window without a prior under gauge none with mu = 0 is rank deficient; a bad mu
    w = _window(cfg, ocfg, seed=33, L=40, prior=False)
    for order in ("dense", "eliminated"):
        st = step_ref.window_step(ocfg, w, 0.0, "none", order=order)
        assert st["status"] == 1 and np.isnan(st["state_step"]).all() and np.isnan(st["lm_step"]).all()
    assert step_ref.window_step(ocfg, w, -1.0, "frame0")["status"] == 1 and step_ref.window_step(ocfg, w, np.nan, "frame0")["status"] == 1
