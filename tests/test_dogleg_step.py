"""CPU: the dogleg step call's C-ABI (symbols, struct sizes and offsets, defaults, argument validation without a device, the binding) and
the definition the GPU pass is held to (tests/dogleg_ref.py): the radii that put every window on every branch and their margins, the FP64
floor of the definition (one-ulp-moved states; the oracle's classes against the compiled reference's), the tie to the oracle's dogleg along
its own trajectory (teacher forcing, as tests/test_branches.py), and the identities of the definition. Measured figures are printed;
dogleg_ref.FLOOR / TIE_MEASURED stand above them."""
import ctypes as C
import os

import numpy as np
import pytest

import dogleg_ref as DR
import step_ref
import test_gn_step as TG
from conftest import ROOT
from oracle import oracle_py as O
from oracle import ref_py as R

GAUGES = ("none", "frame0")


def test_symbols_exported():
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for n in ("vilo_batch_dogleg_step", "vilo_window_dogleg_step", "vilo_last_dogleg_step_ms", "vilo_default_dogleg_opts"):
        assert hasattr(lib, n), n


def test_struct_sizes_and_offsets_match_header():
    from cerberus_amd import _ctypes as T
    assert C.sizeof(T.DoglegOpts) == 32 and C.sizeof(T.WindowDoglegRecord) == 80
    assert [(f, getattr(T.DoglegOpts, f).offset) for f, _ in T.DoglegOpts._fields_] == \
        [("gauge", 0), ("pad0", 4), ("min_lm_diagonal", 8), ("max_lm_diagonal", 16), ("min_pivot", 24)]
    names = [f for f, _ in T.WindowDoglegRecord._fields_]
    assert names == ["alpha", "gradient_norm", "gauss_newton_norm", "step_norm", "beta", "model_cost_change", "grad_dot_step", "norm",
                     "branch", "n_free", "status", "pad"]
    assert [getattr(T.WindowDoglegRecord, f).offset for f in names] == [0, 8, 16, 24, 32, 40, 48, 56, 64, 68, 72, 76]
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    assert "} vilo_dogleg_opts;" in hdr and "} vilo_window_dogleg_record;" in hdr
    # the header's order of the record's fields
    body = hdr[hdr.index("double alpha;"):hdr.index("} vilo_window_dogleg_record;")]
    at = [body.index(f) for f in ("double alpha;", "double gradient_norm;", "double gauss_newton_norm;", "double step_norm;", "double beta;",
                                  "double model_cost_change;", "double grad_dot_step, norm;", "int32_t branch;", "int32_t n_free, status, pad;")]
    assert at == sorted(at)
    src = open(os.path.join(ROOT, "cerberus_amd", "csrc", "kernels_dogleg.hip")).read()
    assert "static_assert(sizeof(vilo_dogleg_opts) == 32" in src and "static_assert(sizeof(vilo_window_dogleg_record) == 80" in src
    assert "offsetof(vilo_window_dogleg_record, branch) == 64" in src and "offsetof(vilo_window_dogleg_record, status) == 72" in src


def test_defaults_and_bad_arguments_without_a_device():
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    L = api.lib()
    o, so = T.DoglegOpts(), T.StepOpts()
    L.vilo_default_dogleg_opts(C.byref(o))
    L.vilo_default_step_opts(C.byref(so))
    assert (o.gauge, o.pad0, o.min_lm_diagonal, o.max_lm_diagonal, o.min_pivot) == (T.COV_GAUGES["none"], 0, 1e-6, 1e32, 1e-14)
    assert bytes(o) == bytes(so)
    L.vilo_default_dogleg_opts(None)
    rec, rad = (T.WindowDoglegRecord * 1)(), (C.c_double * 1)(1.0)
    assert L.vilo_batch_dogleg_step(None, None, None, rad, None, rec, None, None, None, None) == -2
    assert L.vilo_window_dogleg_step(None, 1, None, None, None, rad, None, rec, None, None, None, None) == -2
    assert L.vilo_last_dogleg_step_ms(None) == -1.0


def test_python_binding_present():
    from cerberus_amd import api
    assert callable(getattr(api.Batch, "dogleg_step", None))
    assert callable(getattr(api.Context, "window_dogleg_step", None))
    assert api.DoglegStep._fields == ("state_step", "lm_step", "cauchy_state", "cauchy_lm", "offsets", "alpha", "gradient_norm", "gauss_newton_norm",
                                      "step_norm", "beta", "model_cost_change", "grad_dot_step", "norm", "branch", "n_free", "status")
    import inspect
    p = inspect.signature(api.Batch.dogleg_step).parameters
    assert list(p)[:5] == ["self", "radius", "mu", "gauge", "cauchy"] and p["mu"].default is None and p["cauchy"].default is False


def test_dogleg_step_args_validation():
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    o, rad, mu = api.dogleg_step_args(3, 1e4)
    assert mu is None and rad.tolist() == [1e4] * 3 and rad.flags.c_contiguous and o.gauge == T.COV_GAUGES["none"] and o.min_pivot == 1e-14
    o, rad, mu = api.dogleg_step_args(2, [1.0, 2.0], mu=1e-8, gauge="frame0")
    assert o.gauge == T.COV_GAUGES["frame0"] and rad.tolist() == [1.0, 2.0] and mu.tolist() == [1e-8, 1e-8]
    for bad in (dict(radius=0.0), dict(radius=-1.0), dict(radius=np.nan), dict(radius=np.inf), dict(radius=[1.0, 2.0]), dict(radius=np.ones((3, 1))),
                dict(radius=1.0, mu=-1.0), dict(radius=1.0, gauge="frame1"), dict(radius=1.0, min_pivot=-1.0)):
        with pytest.raises(ValueError):
            api.dogleg_step_args(3, **bad)


# ---- the definition ----
@pytest.fixture(scope="module")
def cases(cfg, ocfg):
    """name -> (window, mu, {gauge: (radii, Gauss-Newton point)}): computed once, shared and left unchanged"""
    out = {}
    for name, (make, mu) in DR.CASES.items():
        w = make(cfg, ocfg)
        sy, per = None, {}
        for gauge in GAUGES:
            with TG._ref():
                per[gauge] = DR.radii(ocfg, w, mu, gauge, sys_=sy)
            sy = per[gauge][1]["sys"]
        out[name] = (w, mu, per)
    return out


def test_radii_put_every_window_on_every_branch_with_margin(cases, ocfg):
    """Delta = 2 |p^_gn|, alpha |g^| / 2, (alpha |g^| + |p^_gn|) / 2: branches 0, 1, 2 for every case under both gauges, every decision of
    the reference at least dogleg_ref.MARGIN (relative) from its threshold; mu = 0 with a prior, 1e-8 without one."""
    worst = np.inf
    for name, (w, mu, per) in cases.items():
        assert mu == (0.0 if w.prior.struct.valid else 1e-8), name
        for gauge in GAUGES:
            rad, gn = per[gauge]
            for want, radius in enumerate(rad):
                r = DR.window_dogleg(ocfg, w, radius, mu, gauge, gn=gn)
                assert r["status"] == 0 and r["branch"] == want, (name, gauge, want, r["branch"])
                worst = min(worst, min(r["margins"]))
                assert min(r["margins"]) >= DR.MARGIN, (name, gauge, want, r["margins"])
    print("MEASURED smallest margin of a branch decision: %.2e (required %.0e)" % (worst, DR.MARGIN))


def test_identities_of_the_definition(cases, ocfg):
    """Under both gauges: |p^| = Delta on branches 1 and 2, the predicted decrease positive and, on branch 1, alpha-limited; the Cauchy
    point minimises the model along its direction; g^T c = c^T M c; held entries zero; delta^T H delta by bilinearity is the product."""
    for name, (w, mu, per) in cases.items():
        for gauge in GAUGES:
            rad, gn = per[gauge]
            sy = gn["sys"]
            H, g, dd = sy["H"], sy["g"], sy["dd"]
            for want, radius in enumerate(rad):
                r = DR.window_dogleg(ocfg, w, radius, mu, gauge, gn=gn)
                d, c = r["delta"], r["c"]
                assert r["model_cost_change"] > 0.0 and r["grad_dot_step"] < 0.0
                assert abs(np.sqrt(dd @ (d * d)) - r["step_norm"]) <= 1e-12 * r["step_norm"]
                if want:
                    assert abs(r["step_norm"] - radius) <= 1e-12 * radius
                assert abs(g @ c - c @ (dd * c)) <= 1e-12 * abs(g @ c)
                a = 0.0 if want == 0 else (-(radius / r["gradient_norm"]) if want == 1 else -r["alpha"] * (1.0 - r["beta"]))
                dn = gn["delta"]
                bil = a * a * (c @ H @ c) + 2.0 * a * r["beta"] * (c @ H @ dn) + r["beta"] ** 2 * (dn @ H @ dn)
                assert abs(bil - d @ H @ d) <= 1e-10 * abs(d @ H @ d)
                if gauge == "frame0":
                    u = __import__("cov_ref").quat_R(w.pose[0, 3:7])[2]
                    for v in (r["state_step"], r["cauchy_state"]):
                        assert not v[:3].any() and abs(u @ v[3:6]) <= 1e-14 * np.abs(v[3:6]).max()
                free = __import__("grad_ref").free_mask(w)
                assert not r["state_step"][~free].any() and not r["cauchy_state"][~free].any()
    w = cases["prior"][0]
    for radius in (0.0, -1.0, np.nan, np.inf):
        assert DR.window_dogleg(ocfg, w, radius, 0.0)["status"] == 1
    assert DR.window_dogleg(ocfg, w, 1.0, np.nan)["status"] == 1


def _ulp_moved(w, rng):
    v = w.twin()
    for a in v.state_arrays():
        a *= 1.0 + np.finfo(float).eps * rng.choice([-1.0, 1.0], size=a.shape)
    return v


def test_fp64_floor_measured(cases, ocfg):
    """The spread of the definition in FP64, the way tests/test_gn_step.py measures step_ref.FLOOR: every state entry moved by one unit in
    the last place (seeded signs), and the oracle's classes against the compiled reference's (where built); every case, both gauges, the
    three radii of the unmoved reference."""
    rng = np.random.default_rng(23)
    fl = {k: 0.0 for k in DR.FLOOR}
    for name, (w, mu, per) in cases.items():
        v = _ulp_moved(w, rng)
        for gauge in GAUGES:
            rad, gn = per[gauge]
            with TG._ref():
                m_gn = step_ref.window_step(ocfg, v, mu, gauge, order="eliminated")
            o_gn = step_ref.window_step(ocfg, w, mu, gauge, order="eliminated") if R.available() else None
            for radius in rad:
                a = DR.window_dogleg(ocfg, w, radius, mu, gauge, gn=gn)
                others = [DR.window_dogleg(ocfg, v, radius, mu, gauge, gn=m_gn)] + ([DR.window_dogleg(ocfg, w, radius, mu, gauge, gn=o_gn)] if o_gn else [])
                for m in others:
                    assert m["status"] == 0 and m["branch"] == a["branch"], (name, gauge, radius)
                    e = DR.errors(gn["sys"], m, a)
                    fl = {k: max(fl[k], e[k]) for k in fl}
                print("MEASURED floor %-14s gauge %-6s branch %d: %s" % (name, gauge, a["branch"], " ".join("%s %.1e" % (k, x) for k, x in e.items())))
    print("MEASURED floor: %s" % {k: "%.1e" % x for k, x in fl.items()})
    print("         FLOOR: %s" % {k: "%.0e" % x for k, x in DR.FLOOR.items()})
    for k, x in fl.items():
        assert x <= DR.FLOOR[k], (k, x, DR.FLOOR[k])


# the oracle's trajectories: (window parameters, initial radius, iterations), tests/test_branches.py's windows of the three dogleg kinds
TRAJECTORIES = ((dict(seed=11), 1e-3, 4), (dict(seed=11), 1e-1, 4), (dict(seed=20, sig_p=0.2, sig_theta=0.08, sig_lambda_rel=0.6, sig_v=0.5), 1e4, 8))


def oracle_trajectory(cfg, ocfg, wkw, radius0, n_iters, mu0=1e-8):
    """Teacher forcing, as tests/test_branches.py::_single_steps: the states (x_i, radius_i, mu_i) the oracle visits, and from each of them
    the scalars (orc_last_step_scalars) of the ONE iteration the oracle takes there. Yields (window at x_i, radius_i, mu_i, scalars)."""
    import test_branches as TB
    O.lib().orc_set_initial_mu.argtypes = [C.c_double]

    def scalars():
        out = (C.c_double * 12)()
        O.lib().orc_last_step_scalars(out)
        return list(out)
    try:
        for i in range(n_iters):
            w = TB._window(cfg, ocfg, **wkw)
            O.lib().orc_set_initial_mu(mu0)
            oo = O.default_opts(True, i)
            oo.initial_trust_region_radius = radius0
            sm = O.solve_window(ocfg, w, oo, check=False)
            sc = scalars()
            radius_i, mu_i = (sm.radius_trace[i], sc[8]) if i else (radius0, mu0)
            if sm.termination == 2:
                break
            at = w.twin()
            o1 = O.default_opts(True, 1)
            o1.initial_trust_region_radius = radius_i
            O.lib().orc_set_initial_mu(mu_i)
            O.solve_window(ocfg, w, o1, check=False)
            yield at, radius_i, mu_i, scalars()
    finally:
        O.lib().orc_set_initial_mu(1e-8)


def tie_errors(r, sc):
    """relative differences of a dogleg result (dict or record fields) against the oracle's scalars"""
    pairs = (("alpha", r["alpha"], sc[0]), ("gnorm2", r["gradient_norm"] ** 2, sc[1]), ("gnnorm2", r["gauss_newton_norm"] ** 2, sc[2]),
             ("model", r["model_cost_change"], sc[3]), ("step_norm", r["step_norm"], sc[6]))
    return {k: abs(a - b) / abs(b) for k, a, b in pairs}


def test_tie_to_the_oracles_trajectory(cfg, ocfg):
    """Along the oracle's own trajectory, from every state it visits: alpha, |g^|^2, |p^_gn|^2, model_cost_change, step_norm and the branch
    of dogleg_ref at the oracle's radius and mu against the oracle's g_last. All three branches must occur."""
    worst, kinds = 0.0, set()
    for wkw, radius0, n in TRAJECTORIES:
        for i, (w, radius, mu, sc) in enumerate(oracle_trajectory(cfg, ocfg, wkw, radius0, n)):
            with TG._ref():
                r = DR.window_dogleg(ocfg, w, radius, mu, "none")
            assert r["status"] == 0 and r["branch"] == int(sc[10]), (wkw, i, r["branch"], sc[10])
            assert (r["model_cost_change"] > 0.0) == (sc[9] >= 0)
            e = tie_errors(r, sc)
            print("MEASURED tie seed %d radius0 %g step %d (radius %.3g mu %.1e branch %d): %s"
                  % (wkw["seed"], radius0, i, radius, mu, r["branch"], " ".join("%s %.1e" % kv for kv in e.items())))
            worst = max(worst, max(e.values()))
            kinds.add(r["branch"])
    print("MEASURED tie: worst %.2e (recorded %.0e, bound %.0e)" % (worst, DR.TIE_MEASURED, DR.TIE_BOUND))
    assert kinds == {0, 1, 2}, kinds
    assert worst <= DR.TIE_BOUND
