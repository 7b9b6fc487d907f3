"""Test helper: the state covariance of a window (include/vilo_gpu.h, "state covariance") in numpy, from ref_gradient.dense_jacobian — the
whitened, loss-corrected Jacobian in local coordinates, independent of the kernels under test — at the window's current state arrays.
Returns the arrays vilo_batch_covariance returns: frames [11][19][19] (dp dtheta v ba bg rho per frame) and poses [79][79] (11 poses, ex0,
ex1, td), zero where a block is constant or absent."""
import numpy as np

from ref_gradient import dense_jacobian


def quat_R(q):
    x, y, z, w = np.asarray(q, float) / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])


def hessian(cfg, w):
    """(H = J^T J over the free blocks, column layout {key: slice}, J)"""
    _, J, cols = dense_jacobian(cfg, w)
    return J.T @ J, cols, J


def gauge_basis(w, cols, n, rot=None):
    """N (n x n-4): frame 0's dp columns removed, its dtheta restricted to the plane orthogonal to u = R0^T e_z. rot: any 3 x 2 orthonormal
    basis of that plane (default: from the SVD)."""
    u = quat_R(w.pose[0, 3:7])[2]
    if rot is None:
        rot = np.linalg.svd(u.reshape(1, 3))[2][1:].T
    s0 = cols[(0, 0)].start
    keep = [i for i in range(n) if not (s0 <= i < s0 + 6)]
    N = np.zeros((n, len(keep) + 2))
    for j, i in enumerate(keep):
        N[i, j] = 1.0
    N[s0 + 3:s0 + 6, len(keep):] = rot
    return N


def equilibrated_inverse(A):
    """A^-1 through the Cholesky factor of D A D (unit diagonal)"""
    d = 1.0 / np.sqrt(np.diag(A))
    L = np.linalg.cholesky(A * d[:, None] * d[None, :])
    Li = np.linalg.inv(L)
    return (Li.T @ Li) * d[:, None] * d[None, :]


def covariance(H, N=None):
    """Sigma = N (N^T H N)^-1 N^T (N None: H^-1)"""
    if N is None:
        return equilibrated_inverse(H)
    return N @ equilibrated_inverse(N.T @ H @ N) @ N.T


def camera_index(cols):
    """camera-side columns: {('f', k, c): column} for c < 19 in the frame order, {('p', i): column} for the 79 pose-system dims"""
    out = {}
    for (kind, idx), sl in cols.items():
        if kind == 0:
            for c in range(6):
                out[("f", idx, c)] = sl.start + c
                out[("p", 6 * idx + c)] = sl.start + c
        elif kind == 1:
            for c in range(9):
                out[("f", idx, 6 + c)] = sl.start + c
        elif kind == 2:
            for c in range(4):
                out[("f", idx, 15 + c)] = sl.start + c
        elif kind == 3:
            for c in range(6):
                out[("p", 66 + 6 * idx + c)] = sl.start + c
        elif kind == 4:
            out[("p", 78)] = sl.start
    return out


def outputs(S, cols):
    """frames [11][19][19], poses [79][79] of a full covariance S over dense_jacobian's columns"""
    ix = camera_index(cols)
    frames, poses = np.zeros((11, 19, 19)), np.zeros((79, 79))
    for k in range(11):
        sel = [(c, ix[("f", k, c)]) for c in range(19) if ("f", k, c) in ix]
        for a, ia in sel:
            for b, ib in sel:
                frames[k, a, b] = S[ia, ib]
    sel = [(p, ix[("p", p)]) for p in range(79) if ("p", p) in ix]
    for a, ia in sel:
        for b, ib in sel:
            poses[a, b] = S[ia, ib]
    return frames, poses


def window_covariance(cfg, w, gauge="frame0"):
    H, cols, _ = hessian(cfg, w)
    N = gauge_basis(w, cols, H.shape[0]) if gauge == "frame0" else None
    return outputs(covariance(H, N), cols)


def scaled_diff(A, B):
    """|A_ij - B_ij| / sqrt(B_ii B_jj) (0 where B's diagonal is 0), per entry; the last two axes are the matrix"""
    d = np.sqrt(np.abs(np.diagonal(B, axis1=-2, axis2=-1)))
    den = d[..., :, None] * d[..., None, :]
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(den > 0, np.abs(A - B) / np.where(den > 0, den, 1.0), 0.0)
    return r


# GPU tolerances per entry, correlation-scaled: ten times the FP64 floor tests/test_covariance.py measures. With a prior: pose / extrinsic /
# td entries 3.8e-6 against 40-digit arithmetic, 2.3e-6 under a one-ulp perturbation of J; speed-bias / rho 1.8e-5. Without a prior (only
# the FRAME0 gauge holds the window; cond ~1e13): 1.6e-4 for every kind under the one-ulp perturbation.
TOL_POSE, TOL_SB = 4e-5, 2e-4
TOL_NO_PRIOR = 2e-3


def tolerances(has_prior):
    """(pose / ex / td, speed-bias / rho)"""
    return (TOL_POSE, TOL_SB) if has_prior else (TOL_NO_PRIOR, TOL_NO_PRIOR)

FRAME_POSE = slice(0, 6)      # dp dtheta rows of a frame block
FRAME_SB = slice(6, 19)       # v ba bg rho rows


def block_errors(frames_a, frames_b, poses_a=None, poses_b=None):
    """worst correlation-scaled difference per kind: 'pose' (dp dtheta rows and columns), 'sb' (every entry with a v ba bg rho row or
    column: the pose <-> speed-bias cross terms count here), 'ex_td' (extrinsic / td rows of the pose system)"""
    e = scaled_diff(frames_a, frames_b)
    out = {"pose": float(e[:, FRAME_POSE, FRAME_POSE].max()), "sb": float(e[:, FRAME_SB, :].max())}
    if poses_a is not None:
        ep = scaled_diff(poses_a, poses_b)
        out["pose"] = max(out["pose"], float(ep[:66].max()))
        out["ex_td"] = float(ep[66:].max())
    return out
