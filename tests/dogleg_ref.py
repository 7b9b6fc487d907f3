"""Test helper: the dogleg trust-region step of a window (include/vilo_gpu.h, "dogleg trust-region step") in numpy, on step_ref's dense H
and g (ref_gradient.dense_jacobian: the factor classes' own Evaluate(); nothing of the kernels under test), in the arrays
vilo_batch_dogleg_step returns. The Gauss-Newton point is step_ref.window_step's; delta^T H delta is a product of its own here, not the
kernel's bilinear form. Under 'frame0' everything lives in the gauge's subspace delta = N z (cov_ref.gauge_basis): the Cauchy direction is
N (N^T M N)^-1 N^T g with M = diag(D^2 / s^2)."""
import numpy as np

import step_ref

NS = step_ref.NS
SCALARS = ("alpha", "gradient_norm", "gauss_newton_norm", "step_norm", "beta", "model_cost_change", "grad_dot_step", "norm")
RECORD = SCALARS + ("branch", "n_free", "status")

# FP64 floors of the definition, as tests/test_dogleg_step.py::test_fp64_floor_measured prints them: the largest figure over CASES x the
# three radii x both gauges of the one-ulp-moved state (and of the oracle's classes against the compiled reference's, where built), rounded
# up. "step" and "cauchy" in step_ref's metric max_i |d delta_i| sqrt(h_i) / |sqrt(h) o delta|_inf, the scalars relative. The GPU bounds are
# ten times these (TOL).
FLOOR = {
    "step": 3e-6, "cauchy": 6e-14, "alpha": 4e-15, "gradient_norm": 3e-14, "gauss_newton_norm": 3e-6, "step_norm": 3e-6, "beta": 4e-6,
    "model_cost_change": 2e-7, "grad_dot_step": 2e-7, "norm": 4e-6,
}   # measured 2.9e-6, 5.0e-14, 3.7e-15, 2.0e-14, 2.1e-6, 2.1e-6, 3.3e-6, 1.1e-7, 1.4e-7, 3.8e-6
TOL = {k: 10.0 * v for k, v in FLOOR.items()}
# every decision of the reference sits at least this far (relative) from its threshold at the radii of radii()
MARGIN = 1e-6

# the oracle tie (tests/test_dogleg_step.py::test_tie_to_the_oracles_trajectory): the largest relative difference measured there on the CPU
# over alpha, |g^|^2, |p^_gn|^2, model_cost_change and step_norm; the bound is ten times it
TIE_MEASURED = 2e-8   # measured 1.47e-8 (|p^_gn|^2 at the last state of the seed-20 trajectory)
TIE_BOUND = 10.0 * TIE_MEASURED

# name -> (maker, mu): the windows of the floor measurement and of the GPU tests. mu = 0 with a prior, 1e-8 without one.
CASES = {
    "prior": (lambda cfg, ocfg: _cw()(cfg, ocfg, seed=1201, L=40), 0.0),
    "no_prior": (lambda cfg, ocfg: _cw()(cfg, ocfg, seed=1202, L=40, prior=False), 1e-8),
    "imu_only": (lambda cfg, ocfg: _cw()(cfg, ocfg, seed=1203, L=40, use_leg=0, leg_bias_const=1), 0.0),
    "many_landmarks": (lambda cfg, ocfg: _cw()(cfg, ocfg, seed=1204, L=300), 0.0),   # more than 256: a thread's second landmark
    "field": (lambda cfg, ocfg: __import__("field_windows").field_window(cfg, ocfg, "f40"), 0.0),
    "const": (lambda cfg, ocfg: __import__("const_windows").leg_window(cfg, ocfg, "c40_ex_td"), 0.0),
    "two_frames": (lambda cfg, ocfg: __import__("frame_windows").leg_window(cfg, ocfg, "g2"), 1e-8),
    "eleven_frames": (lambda cfg, ocfg: __import__("frame_windows").leg_window(cfg, ocfg, "g11"), 1e-8),
}


def _cw():
    from test_covariance_gpu import _window
    return _window


def window_dogleg(cfg, w, radius, mu=0.0, gauge="none", lo=1e-6, hi=1e32, min_pivot=1e-14, sys_=None, gn=None):
    """dict(state_step [222], lm_step [L], cauchy_state, cauchy_lm, the record's fields, delta, cauchy, c, sys, gn, margins)"""
    if gn is None:
        gn = step_ref.window_step(cfg, w, mu, gauge, lo, hi, min_pivot, order="eliminated", sys_=sys_)
    sys_ = gn["sys"]
    out = dict(state_step=np.full(NS, np.nan), lm_step=np.full(w.L, np.nan), cauchy_state=np.full(NS, np.nan), cauchy_lm=np.full(w.L, np.nan),
               branch=-1, n_free=gn["n_free"], status=1, delta=None, sys=sys_, gn=gn)
    out.update({k: np.nan for k in SCALARS})
    if gn["status"] != 0 or not (np.isfinite(radius) and radius > 0.0):
        return out
    H, g, dd = sys_["H"], sys_["g"], sys_["dd"]
    _, _, N = step_ref.reduced(w, sys_, mu, gauge)
    c = g / dd if N is None else N @ np.linalg.solve(N.T @ (dd[:, None] * N), N.T @ g)
    d = gn["delta"]
    gg, cHc = float(g @ c), float(c @ (H @ c))
    alpha, gnorm, gn_norm = gg / cHc, np.sqrt(gg), gn["scaled_norm"]
    margins = [abs(gn_norm - radius) / radius]
    if gn_norm <= radius:
        branch, a, beta = 0, 0.0, 1.0
    else:
        margins.append(abs(gnorm * alpha - radius) / radius)
        if gnorm * alpha >= radius:
            branch, a, beta = 1, -(radius / gnorm), 0.0
        else:
            branch = 2
            b_dot_a = -alpha * float(g @ d)
            a_sq = (alpha * gnorm) ** 2
            bma = a_sq - 2.0 * b_dot_a + gn_norm ** 2
            cc = b_dot_a - a_sq
            dq = np.sqrt(cc * cc + bma * (radius ** 2 - a_sq))
            beta = (dq - cc) / bma if cc <= 0.0 else (radius ** 2 - a_sq) / (dq + cc)
            a = -alpha * (1.0 - beta)
    delta = d.copy() if branch == 0 else a * c + beta * d
    cauchy = -alpha * c
    gd = float(g @ delta)
    step_norm = gn_norm if branch == 0 else (radius if branch == 1 else float(np.sqrt(dd @ (delta * delta))))
    full, fc = np.zeros(NS + w.L), np.zeros(NS + w.L)
    full[sys_["pos"]], fc[sys_["pos"]] = delta, cauchy
    out.update(state_step=full[:NS], lm_step=full[NS:], cauchy_state=fc[:NS], cauchy_lm=fc[NS:], alpha=alpha, gradient_norm=gnorm,
               gauss_newton_norm=gn_norm, step_norm=step_norm, beta=beta, model_cost_change=-(gd + 0.5 * float(delta @ (H @ delta))),
               grad_dot_step=gd, norm=float(np.linalg.norm(delta)), branch=branch, status=0, delta=delta, cauchy=cauchy, c=c,
               margins=margins)
    return out


def radii(cfg, w, mu, gauge, sys_=None):
    """(radius of branch 0, of branch 1, of branch 2, the Gauss-Newton point) from the reference alone: 2 |p^_gn|, alpha |g^| / 2 and
    (alpha |g^| + |p^_gn|) / 2"""
    r = window_dogleg(cfg, w, 1.0, mu, gauge, sys_=sys_)
    assert r["status"] == 0
    ca, gn = r["alpha"] * r["gradient_norm"], r["gauss_newton_norm"]
    return (2.0 * gn, 0.5 * ca, 0.5 * (ca + gn)), r["gn"]


def errors(sys_, got, ref):
    """{field: error} of two window_dogleg-shaped results (ref of status 0): the steps in step_ref's metric, the scalars relative"""
    e = {"step": step_ref.step_error(sys_, got["delta"], ref["delta"])}
    if got.get("cauchy") is not None:
        e["cauchy"] = step_ref.step_error(sys_, got["cauchy"], ref["cauchy"])
    for k in SCALARS:
        e[k] = abs(got[k] - ref[k]) / abs(ref[k]) if ref[k] != 0.0 else abs(got[k])
    return e
