"""Test helper (no test in it): the definition of vilo_batch_retract (include/vilo_gpu.h, "caller-given local steps") in numpy, on a
window's state arrays. s = alpha * step and x + s are single numpy operations, so each is rounded once, as the kernel rounds them; the
pose and extrinsic blocks go through a pose_plus the caller hands in (the oracle's on a CPU, Context.pose_plus on the GPU, which the
kernel's blocks must equal to the bit) or through pose_plus_np, PoseLocalParameterization::Plus written out in numpy.
Layout of the 222 step entries: vilo_batch_gradient's (grad_ref.BLOCKS)."""
import numpy as np

import grad_ref

NS = grad_ref.NS
OK, NUMERIC = 0, 1   # vilo_window_retract_record.status


def pose_plus_np(x, s):
    """[n, 7] x [n, 6] -> [n, 7]: p + dp, (q * deltaQ(dtheta)).normalized() with deltaQ = (1, dtheta / 2) (utility.h:28-41), the
    quaternion stored x y z w. Eigen's product, term by term in its order; no claim to the last bit."""
    x, s = np.atleast_2d(np.asarray(x, float)), np.atleast_2d(np.asarray(s, float))
    out = np.empty_like(x)
    out[:, :3] = x[:, :3] + s[:, :3]
    ax, ay, az, aw = x[:, 3], x[:, 4], x[:, 5], x[:, 6]
    bx, by, bz, bw = s[:, 3] / 2.0, s[:, 4] / 2.0, s[:, 5] / 2.0, 1.0
    w = aw * bw - ax * bx - ay * by - az * bz
    qx = aw * bx + ax * bw + ay * bz - az * by
    qy = aw * by + ay * bw + az * bx - ax * bz
    qz = aw * bz + az * bw + ax * by - ay * bx
    n = np.sqrt(w * w + qx * qx + qy * qy + qz * qz)
    out[:, 3], out[:, 4], out[:, 5], out[:, 6] = qx / n, qy / n, qz / n, w / n
    return out


def applied(w, lm_mask=None):
    """(state [222] bool, landmarks [L] bool): the coordinates a step moves. The state part is the gradient's free set."""
    lm = np.ones(w.L, bool) if lm_mask is None else ~(np.asarray(lm_mask) != 0)
    return grad_ref.free_mask(w), lm


def retract(w, state_step, lm_step, alpha, pose_plus=pose_plus_np, lm_mask=None, base=None):
    """The state arrays [pose, speed_bias, leg_bias, ex_pose, td, inv_depth] after the step and the record dict(status, n_applied,
    step_norm, step_max). base: the arrays stepped (default: w's own). Entries that are not applied are copied, whatever the step holds
    there; a non-finite alpha or applied s leaves everything as it is (NUMERIC, the record's numbers 0)."""
    base = w.state_arrays() if base is None else base
    out = [np.array(a, dtype=np.float64, copy=True) for a in base]
    fs, fl = applied(w, lm_mask)
    alpha = np.float64(alpha)
    with np.errstate(invalid="ignore", over="ignore"):
        s = alpha * np.asarray(state_step, np.float64)
        sl = alpha * np.asarray(lm_step, np.float64)
    sv = np.concatenate([s[fs], sl[fl]])
    if not (np.isfinite(alpha) and np.isfinite(sv).all()):
        return out, dict(status=NUMERIC, n_applied=0, step_norm=0.0, step_max=0.0)
    rec = dict(status=OK, n_applied=int(sv.size), step_norm=float(np.sqrt(np.sum(sv * sv))), step_max=float(np.abs(sv).max()) if sv.size else 0.0)
    F = w.F
    # pose and extrinsic blocks, in one call
    blocks = [(0, k) for k in range(F)] + [(3, c) for c in range(2) if fs[grad_ref.position(3, c)]]
    if blocks:
        X = np.array([out[a][i] for a, i in blocks])
        S = np.array([s[grad_ref.position(a, i):grad_ref.position(a, i) + 6] for a, i in blocks])
        P = np.asarray(pose_plus(X, S))
        for (a, i), p in zip(blocks, P):
            out[a][i] = p
    for k in range(F):
        out[1][k] = out[1][k] + s[grad_ref.position(1, k):grad_ref.position(1, k) + 9]
        if fs[grad_ref.position(2, k)]:
            out[2][k] = out[2][k] + s[grad_ref.position(2, k):grad_ref.position(2, k) + 4]
    if fs[grad_ref.position(4, 0)]:
        out[4][0] = out[4][0] + s[grad_ref.position(4, 0)]
    out[5][fl] = out[5][fl] + sl[fl]
    return out, rec


def random_step(w, rng, scale=1e-2, lm_mask=None, poison=np.nan):
    """(state_step [222], lm_step [L]): normal entries of size `scale` on the applied coordinates, `poison` on every other one (constant
    blocks, absent frames, masked landmarks: the call must not read them)."""
    fs, fl = applied(w, lm_mask)
    s, sl = scale * rng.normal(size=NS), scale * rng.normal(size=w.L)
    s[~fs] = poison
    sl[~fl] = poison
    return s, sl


# ---- the windows the retract tests share, by kind ----
# leg windows (one batch kind), in the order a batch of five holds them: 8 frames and ragged tracks; a free td; constant extrinsics; constant
# leg biases; 2 frames (constant extrinsics and leg biases, no prior)
LEG_KINDS = ("f60_partial8", "f40_td", "c40_ex", "c40_lb", "g2")
IMU_KIND = "v130_noprior"   # use_leg == 0: a batch of its own (a batch holds one IMU factor kind)


def kind_window(cfg, ocfg, name):
    import const_windows as CW
    import field_windows as FW
    import frame_windows as GW
    if name in FW.RECIPES:
        return FW.field_window(cfg, ocfg, name)
    if name in CW.LEG:
        return CW.leg_window(cfg, ocfg, name)
    if name in CW.VINS:
        return CW.vins_window(cfg, ocfg, name)
    return GW.make(cfg, ocfg, name)


def batch_of(S, W, kinds=LEG_KINDS):
    """W windows: the kinds in turn, twins of S's windows (S itself is never uploaded, so it keeps its start state)."""
    return [S[kinds[p % len(kinds)]].twin() for p in range(W)]


# ---- directional derivative of the cost along a unit direction over the free coordinates ----
# Measured with the oracle's cost and numpy's gradient, |dd - g.d| / |g|, largest over the window kinds: 4.3e-11 at 1e-4 (the 2-frame window
# 3.9e-11 against 2e-13 one step down: truncation begins), 2.6e-10 at 1e-5, 8.5e-10 at 1e-6, 4.0e-8 at 1e-7, 2.0e-7 at 1e-8: below 1e-5 the
# error is the cost's rounding (1e10 x 1e-16) over 2 eps and grows as 1 / eps; at 1e-5 truncation is not yet visible on any kind.
EPS = 1e-5


def unit_direction(w, rng):
    """(state [222], landmarks [L]): a random direction of norm 1 over the coordinates a step moves, zero elsewhere"""
    fs, fl = applied(w)
    ds, dl = rng.normal(size=NS) * fs, rng.normal(size=w.L) * fl
    n = np.sqrt((ds * ds).sum() + (dl * dl).sum())
    return ds / n, dl / n


def central_difference(cost_at, eps):
    """(cost(x [+] eps d) - cost(x [+] -eps d)) / (2 eps); cost_at(alpha) is the cost after the step alpha * d from x"""
    return (cost_at(eps) - cost_at(-eps)) / (2.0 * eps)


def dd_error(dd, gd, g_norm):
    """|central difference - g . d| in units of |g| (d is a unit vector, so |g . d| <= |g|)"""
    return abs(dd - gd) / g_norm


# |dd - g.d| / |g| with the oracle's cost and numpy's gradient at EPS, the largest over the window kinds, as
# tests/test_retract.py::test_directional_derivative_with_the_oracle_alone measures it (it holds ten times this, against the seed); the GPU
# test holds ten times the figure, for its other order of summation
DD_MEASURED = 2.7e-10
DD_TOL = 10.0 * DD_MEASURED
DD_SEED = 77   # of unit_direction's generator, in both tests

# pose_plus_np against the oracle's PoseLocalParameterization::Plus (pinned to the reference's in tests/test_oracle_vs_reference.py), largest
# absolute difference over 6000 random poses and steps of size 1e-2, 1e-1 and 1: measured 3.4e-16 (tests/test_retract.py holds ten times it)
PLUS_MEASURED = 3.4e-16
PLUS_TOL = 10.0 * PLUS_MEASURED


def ulps(a, b):
    """|a - b| in units of b's last place"""
    return abs(a - b) / np.spacing(abs(b)) if b != 0 else (0.0 if a == 0 else np.inf)
