"""Test helper: Gauss-Newton Hessian-vector products of a window (include/vilo_gpu.h, "Gauss-Newton Hessian-vector products") in numpy,
H v = J^T (J v) on ref_gradient.dense_jacobian — the factor classes' own Evaluate(), the oracle's or inside `with ref_py.as_oracle():` the
compiled reference's; nothing of the kernels under test — in the arrays vilo_batch_hessian_vector takes and returns (grad_ref's layout: 222
state entries, then the landmarks in the window's own order; step_ref.positions / columns map them to dense_jacobian's columns).
The metric is a matrix-vector product's componentwise bound: e = max_i |dy_i| / ((|J|^T |J|) |v|)_i over the free coordinates; the scalars
vHv and g . v in the same relative measure, |d vHv| / (|v|^T |J|^T |J| |v|) and |d g.v| / ((|J|^T |r|)^T |v|). A free coordinate whose
denominator is zero (a unit vector's product is sparse) is one no Jacobian row couples to v: the product there is exactly zero in any
order of the sums, and anything else counts as an infinite error."""
import numpy as np

import grad_ref
import ref_gradient as RG
import step_ref

NS = grad_ref.NS

# FP64 floor of the definition in the metric above, as tests/test_hess_vec.py::test_fp64_floor_measured prints it (the largest figure over
# its windows and vectors of the one-ulp-moved state and of the oracle's classes against the compiled reference's, rounded up), and the
# GPU bound: ten times it. FLOOR: the products; FLOOR_VHV, FLOOR_GV: the record's scalars. g . v has a figure per class of state: at a solved
# state g is what is left of sums that cancel, and one ulp of the state moves it by H dx, which |J|^T |r| (small there) does not measure.
FLOOR = 7e-13      # measured 6.8e-13 (L 40, prior, solved state: the one-ulp-moved state)
FLOOR_VHV = 7e-14  # measured 6.7e-14 (L 40, prior, initial state: the one-ulp-moved state)
FLOOR_GV = {"initial": 2e-13, "solved": 4e-2}   # measured 1.9e-13 and 3.4e-2 (L 40, no prior, solved: the one-ulp-moved state)
# The solved figure is the conditioning of g in the state, not an error a kernel can show: the GPU test linearises the very bits it
# downloaded. What two implementations at the same bits differ by there is the oracle's classes against the compiled reference's, and
# the GPU's g . v at a solved state is held to ten times that (it comes out at the initial state's figure).
FLOOR_GV_SOLVED_SAME_BITS = 2e-13   # measured 1.7e-13 (L 120, prior, solved: the oracle against the compiled reference)
TOL = 10 * FLOOR
TOL_VHV = 10 * FLOOR_VHV


def tol_gv(solved):
    return 10 * (FLOOR_GV_SOLVED_SAME_BITS if solved else FLOOR_GV["initial"])


def system(cfg, w):
    """dict(J, r, g, aJ = |J|, cols, pos) of window w at its state arrays"""
    r, J, cols = RG.dense_jacobian(cfg, w)
    return dict(J=J, r=r, g=J.T @ r, aJ=np.abs(J), cols=cols, pos=step_ref.positions(w, cols, J.shape[1]))


def columns(sy, state_vec, lm_vec):
    """one vector of the call's arrays ([222], [L]) -> dense_jacobian's column order (entries that are not free are dropped: not read)"""
    return np.concatenate([state_vec, lm_vec])[sy["pos"]]


def arrays(sy, y, L):
    """a vector in dense_jacobian's column order -> (state [222], lm [L]); every other entry zero"""
    full = np.zeros(NS + L)
    full[sy["pos"]] = y
    return full[:NS], full[NS:]


def hess_vec(sy, v):
    return sy["J"].T @ (sy["J"] @ v)


def record(sy, v):
    """(vHv, g_dot_v, model_cost_change) of the definition"""
    jv = sy["J"] @ v
    vhv, gv = float(jv @ jv), float(sy["g"] @ v)
    return vhv, gv, -gv - 0.5 * vhv


def bound(sy, v):
    return sy["aJ"].T @ (sy["aJ"] @ np.abs(v))


def error(sy, got, v, ref=None):
    """e of the product `got` (dense_jacobian's column order) of v in the system sy"""
    ref = hess_vec(sy, v) if ref is None else ref
    den, d = bound(sy, v), np.abs(got - ref)
    if (d[den == 0.0] != 0.0).any():
        return float("inf")
    return float((d[den > 0.0] / den[den > 0.0]).max()) if (den > 0.0).any() else 0.0


def scalar_errors(sy, v, vhv, gv):
    """the relative measures of vHv and g . v against the definition's"""
    r_vhv, r_gv, _ = record(sy, v)
    av = np.abs(v)
    d_vhv, d_gv = float(av @ bound(sy, v)), float((sy["aJ"].T @ np.abs(sy["r"])) @ av)
    return (abs(vhv - r_vhv) / d_vhv if d_vhv > 0 else abs(vhv - r_vhv)), (abs(gv - r_gv) / d_gv if d_gv > 0 else abs(gv - r_gv))


def test_vectors(sy, seed, unit=True):
    """dict name -> vector (dense_jacobian's column order): seeded random (entries of order one, scaled by 1 / sqrt(h) so that no block
    kind drowns the others), -g, and with unit=True a unit vector on one coordinate of every block kind and a landmark-only vector"""
    rng = np.random.default_rng(seed)
    n = sy["J"].shape[1]
    h = (sy["J"] ** 2).sum(axis=0)
    out = {"random": rng.normal(size=n) / np.sqrt(np.where(h > 0, h, 1.0)), "random_plain": rng.normal(size=n), "minus_g": -sy["g"]}
    if unit:
        for key, sl in sy["cols"].items():
            name = "unit_kind%d" % key[0]
            if name not in out:
                e = np.zeros(n)
                e[sl.start + (sl.stop - sl.start) // 2] = 1.0
                out[name] = e
        lm = np.zeros(n)
        for key, sl in sy["cols"].items():
            if key[0] == 9:
                lm[sl] = rng.normal(size=sl.stop - sl.start)
        if lm.any():
            out["landmarks_only"] = lm
    return out
