"""Test helper: the Gauss-Newton / damped step of a window (include/vilo_gpu.h, "Gauss-Newton / damped step") in numpy, on
ref_gradient.dense_jacobian — the factor classes' own Evaluate(), the oracle's or inside `with ref_py.as_oracle():` the compiled
reference's; nothing of the kernels under test — in the arrays vilo_batch_gauss_newton_step returns (grad_ref's layout: 222 state entries,
then the landmarks in the window's own order).
  window_step(..., order="dense")       one equilibrated Cholesky solve of the whole system, no Schur elimination
  window_step(..., order="eliminated")  the kernel's order: inverse depths first, then the speed / bias part, then the pose system
Both solve N^T (H + mu diag(D^2 / s^2)) N z = -N^T g, delta = N z (N = identity under gauge 'none', cov_ref.gauge_basis under 'frame0')."""
import numpy as np

import cov_ref
import grad_ref
import ref_gradient as RG

NS = grad_ref.NS

# FP64 floors of the definition, as tests/test_gn_step.py::test_fp64_floor_measured prints them (the largest figure over its windows of
# the one-ulp-moved state and of the oracle's classes against the compiled reference's, rounded up), and the GPU bounds: ten times them.
#   FLOOR      max_i |d delta_i| sqrt(h_i) / |sqrt(h) o delta|_inf
#   eta        componentwise backward error max_i |(A z + b)_i| / (sum_j |A_ij| |z_j| + |b_i|)
FLOOR = 3e-4   # measured 2.9e-4 (no prior, FRAME0, mu 0: the oracle's classes against the reference's)
TOL = 10 * FLOOR
# eta of the elimination-order numpy solve in its own system: measured 1.2e-15. Ten times it, 2e-14, is what a kernel that solved the
# reference's own H and g could be held to. The device forms H and g itself, in another order of the sums, and its step is measured in the
# reference's system; so the bound per class of case is ten times eta of a step of the one-ulp-moved problem (or of the oracle's classes)
# in the unmoved reference system, each class with its own figure:
ETA_OWN = 2e-15
ETA_FLOORS = {
    "initial": 3e-13,                 # measured 2.5e-13: every case at the initial state
    "solved": 6e-11,                  # measured 5.8e-11: solved state, with a prior (mu 0, 1e-8) or without one under FRAME0 (mu 0)
    "solved_no_prior_damped": 2e-6,   # measured 1.8e-6: solved state, no prior, gauge none, mu 1e-4 (g ~ 0 against |A||z|)
}


def eta_class(solved, prior, mu, gauge):
    if not solved:
        return "initial"
    return "solved_no_prior_damped" if (not prior and gauge == "none" and mu > 0.0) else "solved"


def tol_eta(cls):
    return 10 * ETA_FLOORS[cls]


def positions(w, cols, n):
    """output index (0 .. 221 state entry, 222 + l landmark) of every column of dense_jacobian's layout"""
    pos = np.zeros(n, int)
    for key, sl in cols.items():
        first = NS + key[1] if key[0] == 9 else grad_ref.position(key[0], key[1])
        pos[sl] = first + np.arange(sl.stop - sl.start)
    return pos


def _chol_solve(A, b, min_pivot):
    """x with A x = b through the Cholesky factor of the Jacobi-equilibrated A (unit diagonal); None where a pivot is <= min_pivot"""
    dg = np.diag(A)
    if not (np.isfinite(A).all() and np.isfinite(b).all() and (dg > 0).all()):
        return None
    d = 1.0 / np.sqrt(dg)
    try:
        L = np.linalg.cholesky(A * d[:, None] * d[None, :])
    except np.linalg.LinAlgError:
        return None
    if (np.diag(L) ** 2 <= min_pivot).any():
        return None
    return d * np.linalg.solve(L.T, np.linalg.solve(L, d * b))


def _eliminated_solve(A, b, kinds, min_pivot):
    """the same solution in the kernel's order. kinds: per column 'l' inverse depth, 'b' speed / bias / leg bias, 'p' pose / extrinsic / td"""
    il, ib, ip = (np.flatnonzero(kinds == k) for k in "lbp")
    ic = np.concatenate([ib, ip])
    E = np.diag(A)[il]
    if il.size and not (E > 0).all():
        return None
    W = A[np.ix_(ic, il)]
    Ac = A[np.ix_(ic, ic)] - (W / E) @ W.T
    bc = b[ic] - W @ (b[il] / E)
    dg = np.diag(Ac)
    if not (np.isfinite(Ac).all() and np.isfinite(bc).all() and (dg > 0).all()):
        return None
    d = 1.0 / np.sqrt(dg)
    Ac, bc = Ac * d[:, None] * d[None, :], bc * d
    nb = ib.size
    try:
        LB = np.linalg.cholesky(Ac[:nb, :nb]) if nb else np.zeros((0, 0))
        Y = np.linalg.solve(LB, Ac[:nb, nb:]) if nb else np.zeros((0, ip.size))
        yB = np.linalg.solve(LB, bc[:nb]) if nb else np.zeros(0)
        LP = np.linalg.cholesky(Ac[nb:, nb:] - Y.T @ Y)
    except np.linalg.LinAlgError:
        return None
    if (np.diag(LB) ** 2 <= min_pivot).any() or (np.diag(LP) ** 2 <= min_pivot).any():
        return None
    xP = np.linalg.solve(LP.T, np.linalg.solve(LP, bc[nb:] - Y.T @ yB))
    xB = np.linalg.solve(LB.T, yB - Y @ xP) if nb else np.zeros(0)
    xc = d * np.concatenate([xB, xP])
    x = np.zeros(A.shape[0])
    x[ic] = xc
    x[il] = (b[il] - W.T @ xc) / E
    return x


def linear_system(cfg, w, lo=1e-6, hi=1e32):
    """dict(H, g, dd = D^2 / s^2, h, cols, pos, kinds) of window w at its state arrays"""
    r, J, cols = RG.dense_jacobian(cfg, w)
    H, g = J.T @ J, J.T @ r
    h = np.diag(H).copy()
    s = 1.0 / (1.0 + np.sqrt(h))
    dd = np.clip(s * s * h, lo, hi) / (s * s)
    kinds = np.empty(H.shape[0], "U1")
    for key, sl in cols.items():
        kinds[sl] = "l" if key[0] == 9 else ("b" if key[0] in (1, 2) else "p")
    return dict(H=H, g=g, dd=dd, h=h, cols=cols, pos=positions(w, cols, H.shape[0]), kinds=kinds)


def reduced(w, sys_, mu, gauge):
    """(M, rhs, N): M z = -rhs is the system the step solves; delta = N z (N None: the identity)"""
    A = sys_["H"] + mu * np.diag(sys_["dd"])
    if gauge == "frame0":
        N = cov_ref.gauge_basis(w, sys_["cols"], A.shape[0])
        return N.T @ A @ N, N.T @ sys_["g"], N
    return A, sys_["g"], None


def backward_error(w, sys_, mu, gauge, delta):
    """componentwise backward error of the step `delta` (dense_jacobian's column order) in the system of sys_"""
    M, rhs, N = reduced(w, sys_, mu, gauge)
    z = delta if N is None else N.T @ delta
    den = np.abs(M) @ np.abs(z) + np.abs(rhs)
    return float((np.abs(M @ z + rhs) / den).max())


def columns(w, sys_, state_step, lm_step):
    """the arrays of a step call -> one vector in dense_jacobian's column order"""
    full = np.concatenate([state_step, lm_step])
    return full[sys_["pos"]]


def window_step(cfg, w, mu=0.0, gauge="none", lo=1e-6, hi=1e32, min_pivot=1e-14, order="dense", sys_=None):
    """dict(state_step [222], lm_step [L], model_cost_change, scaled_norm, norm, grad_dot_step, n_free, status, delta, sys)"""
    if sys_ is None:
        sys_ = linear_system(cfg, w, lo, hi)
    n = sys_["H"].shape[0]
    out = dict(state_step=np.full(NS, np.nan), lm_step=np.full(w.L, np.nan), model_cost_change=np.nan, scaled_norm=np.nan, norm=np.nan,
               grad_dot_step=np.nan, n_free=n - (4 if gauge == "frame0" else 0), status=1, delta=None, sys=sys_)
    if not (np.isfinite(mu) and mu >= 0.0):
        return out
    M, rhs, N = reduced(w, sys_, mu, gauge)
    if order == "dense":
        z = _chol_solve(M, -rhs, min_pivot)
    else:
        kinds = sys_["kinds"]
        if N is not None:   # (gauge_basis: the kept identity columns in order, then the two rotation directions of frame 0)
            s0 = sys_["cols"][(0, 0)].start
            kinds = np.concatenate([np.delete(kinds, np.arange(s0, s0 + 6)), ["p", "p"]])
        z = _eliminated_solve(M, -rhs, kinds, min_pivot)
    if z is None or not np.isfinite(z).all():
        return out
    delta = z if N is None else N @ z
    g, dd = sys_["g"], sys_["dd"]
    gd, sdd = float(g @ delta), float(dd @ (delta * delta))
    full = np.zeros(NS + w.L)
    full[sys_["pos"]] = delta
    out.update(state_step=full[:NS], lm_step=full[NS:], model_cost_change=-0.5 * gd + 0.5 * mu * sdd, scaled_norm=np.sqrt(sdd),
               norm=float(np.linalg.norm(delta)), grad_dot_step=gd, status=0, delta=delta)
    return out


def step_error(sys_, got, ref):
    """max_i |d delta_i| sqrt(h_i) / |sqrt(h) o delta|_inf of two steps in dense_jacobian's column order (h, delta of the reference)"""
    sh = np.sqrt(sys_["h"])
    den = np.abs(sh * ref).max()
    return float((np.abs(got - ref) * sh).max() / den) if den > 0 else 0.0
