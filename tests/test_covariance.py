"""CPU: the covariance C-ABI (symbols, struct layout, defaults), the definition the GPU pass is held to (tests/cov_ref.py), and the FP64
floor of that definition measured on synthetic config-2 windows (with a prior: pose entries ~4e-6, speed-bias / rho ~2e-5; without: ~2e-4) — the GPU tolerances of tests/test_covariance_gpu.py must not be tighter."""
import ctypes as C
import os

import numpy as np
import pytest

import cov_ref
from conftest import ROOT
from oracle import oracle_py as O


def test_symbols_exported():
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for n in ("vilo_batch_covariance", "vilo_window_covariance", "vilo_default_cov_opts", "vilo_last_covariance_ms"):
        assert hasattr(lib, n), n


def test_cov_opts_layout_and_defaults():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    assert C.sizeof(T.CovOpts) == 24   # int32 gauge, pad, double min_reciprocal_condition, int32 want_poses, pad (vilo_gpu.h)
    assert T.CovOpts.min_reciprocal_condition.offset == 8 and T.CovOpts.want_poses.offset == 16
    o = api.default_cov_opts()
    assert (o.gauge, o.min_reciprocal_condition, o.want_poses) == (0, 1e-14, 0)
    assert T.COV_GAUGES == {"frame0": 0, "none": 1}


def _solved_window(cfg, ocfg, seed, L, prior):
    from cerberus_amd import synth
    w = synth.make_window(cfg, params=synth.default_params(n_landmarks=L, seed=seed, with_prior=prior))
    O.fill_preint(ocfg, w)
    O.solve_window(ocfg, w, O.default_opts(True, 6))
    return w


@pytest.fixture(scope="module")
def win_prior(cfg, ocfg):
    return _solved_window(cfg, ocfg, 20260925, 120, True)


@pytest.fixture(scope="module")
def win_free(cfg, ocfg):
    return _solved_window(cfg, ocfg, 20260926, 120, False)


def test_frame0_gauge_definition(ocfg, win_free):
    """Sigma = N (N^T H N)^-1 N^T does not depend on N, is the limit of (H + t C^T C)^-1 with C frame 0's position and world-yaw rows, and
    has zero frame-0 position rows."""
    w = win_free
    H, cols, _ = cov_ref.hessian(ocfg, w)
    n = H.shape[0]
    u = cov_ref.quat_R(w.pose[0, 3:7])[2]
    S1 = cov_ref.covariance(H, cov_ref.gauge_basis(w, cols, n))
    rot = cov_ref.gauge_basis(w, cols, n)[cols[(0, 0)].start + 3:cols[(0, 0)].start + 6, -2:]
    c, s = np.cos(0.7), np.sin(0.7)
    S2 = cov_ref.covariance(H, cov_ref.gauge_basis(w, cols, n, rot=rot @ np.array([[c, -s], [s, c]]) @ np.diag([1.0, -1.0])))
    f1, p1 = cov_ref.outputs(S1, cols)
    f2, p2 = cov_ref.outputs(S2, cols)
    e = cov_ref.block_errors(f2, f1, p2, p1)
    assert max(e.values()) < 1e-6, e
    # the constrained limit
    s0 = cols[(0, 0)].start
    Cm = np.zeros((4, n))
    Cm[0:3, s0:s0 + 3] = np.eye(3)
    Cm[3, s0 + 3:s0 + 6] = u
    scale = np.diag(H)[s0:s0 + 6].max()   # (t in units of frame 0's own curvature)
    St = cov_ref.equilibrated_inverse(H + 1e8 * scale * (Cm.T @ Cm))
    ft, pt = cov_ref.outputs(St, cols)
    et = cov_ref.block_errors(ft, f1, pt, p1)
    print("penalty limit at t = 1e8:", {k: "%.1e" % v for k, v in et.items()})
    assert max(et.values()) < 1e-3, et   # (measured 6.5e-5: the penalised matrix's own conditioning, 1e13 x t, is what limits it)
    assert np.abs(f1[0, :3, :]).max() == 0.0 and np.abs(p1[:3, :]).max() == 0.0
    # frame 0's rotation block has rank 2 (u is its null vector)
    assert np.linalg.norm(f1[0, 3:6, 3:6] @ u) < 1e-9 * np.linalg.norm(f1[0, 3:6, 3:6])


def _schur_route(H, cols, N=None):
    """the second FP64 route: landmarks eliminated first (their block is diagonal), the reduced camera system inverted by LU"""
    lam = sorted(sl.start for key, sl in cols.items() if key[0] == 9)
    m = lam[0] if lam else H.shape[0]
    A, B, E = H[:m, :m], H[:m, m:], np.diag(H[m:, m:])
    S = A - (B / E) @ B.T
    n = H.shape[0]
    if N is not None:
        Nc = N[:m, :]
        keep = np.abs(Nc).sum(axis=0) > 0
        Nc = Nc[:, keep]
        d = 1.0 / np.sqrt(np.diag(Nc.T @ S @ Nc))
        Sc = Nc @ (np.linalg.inv((Nc.T @ S @ Nc) * np.outer(d, d)) * np.outer(d, d)) @ Nc.T
    else:
        d = 1.0 / np.sqrt(np.diag(S))
        Sc = np.linalg.inv(S * np.outer(d, d)) * np.outer(d, d)
    out = np.zeros((n, n))
    out[:m, :m] = Sc
    return out


def _floor(ocfg, w, gauge, rng):
    H, cols, J = cov_ref.hessian(ocfg, w)
    N = cov_ref.gauge_basis(w, cols, H.shape[0]) if gauge == "frame0" else None
    S = cov_ref.covariance(H, N)
    f, p = cov_ref.outputs(S, cols)
    f2, p2 = cov_ref.outputs(_schur_route(H, cols, N), cols)
    routes = cov_ref.block_errors(f2, f, p2, p)
    Jp = J * (1.0 + np.finfo(float).eps * rng.choice([-1.0, 1.0], size=J.shape))
    f3, p3 = cov_ref.outputs(cov_ref.covariance(Jp.T @ Jp, N), cols)
    ulp = cov_ref.block_errors(f3, f, p3, p)
    return routes, ulp, (H, cols, N, f, p)


def test_fp64_floor_measured(ocfg, win_prior, win_free):
    """The spread of the definition in FP64 by kind of row, two routes and a one-ulp perturbation of J, for a window with a prior (both
    gauges) and one without (FRAME0). The GPU tolerances (cov_ref.tolerances) must stand above every figure."""
    rng = np.random.default_rng(5)
    rows = []
    for name, w, g in (("prior", win_prior, "frame0"), ("prior", win_prior, "none"), ("no_prior", win_free, "frame0")):
        routes, ulp, _ = _floor(ocfg, w, g, rng)
        rows.append((name, g, routes, ulp))
        print("%-8s %-6s routes %s  one-ulp J %s" % (name, g, {k: "%.1e" % v for k, v in routes.items()}, {k: "%.1e" % v for k, v in ulp.items()}))
        tp, ts = cov_ref.tolerances(name == "prior")
        for e in (routes, ulp):
            assert e["pose"] < tp and e["ex_td"] < tp and e["sb"] < ts, (name, g, e)


def test_fp64_floor_against_exact(cfg, ocfg):
    """One small window: the FP64 route against the covariance of the same FP64 H in 40-digit arithmetic (mpmath)."""
    mp = pytest.importorskip("mpmath")
    w = _solved_window(cfg, ocfg, 4242, 24, True)
    H, cols, _ = cov_ref.hessian(ocfg, w)
    N = cov_ref.gauge_basis(w, cols, H.shape[0])
    f, p = cov_ref.outputs(cov_ref.covariance(H, N), cols)
    with mp.workdps(40):
        A = N.T @ H @ N   # (N's entries are exact in FP64 up to the 3 x 2 rotation block; the same A enters both routes)
        d = 1.0 / np.sqrt(np.diag(A))
        Am = mp.matrix((A * np.outer(d, d)).tolist())
        Ai = mp.inverse(Am)
        Ae = np.array(Ai.tolist(), dtype=np.float64) * np.outer(d, d)
    fe, pe = cov_ref.outputs(N @ Ae @ N.T, cols)
    e = cov_ref.block_errors(f, fe, p, pe)
    print("against 40 digits:", {k: "%.1e" % v for k, v in e.items()})
    assert e["pose"] < cov_ref.TOL_POSE and e["ex_td"] < cov_ref.TOL_POSE and e["sb"] < cov_ref.TOL_SB, e
