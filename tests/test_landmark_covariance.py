"""CPU: the landmark-covariance C-ABI (symbols), the definition the GPU pass is held to (tests/lm_cov_ref.py: the landmark rows of the full
inverse, inverse depths kept), its elimination form from E, w and Sigma_PP, the point Jacobian, and the FP64 floor of the definition
measured on synthetic config-2 windows — the GPU tolerances of tests/test_landmark_covariance_gpu.py (lm_cov_ref.tolerances) must stand
above it."""
import ctypes as C
import os

import numpy as np
import pytest

import cov_ref
import lm_cov_ref
from conftest import ROOT
from oracle import oracle_py as O


def test_symbols_exported():
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for n in ("vilo_batch_landmark_covariance", "vilo_window_landmark_covariance"):
        assert hasattr(lib, n), n


def test_python_binding_present():
    from cerberus_amd import api
    assert callable(getattr(api.Batch, "landmark_covariance", None))
    assert callable(getattr(api.Context, "window_landmark_covariance", None))


def _solved_window(cfg, ocfg, seed, L, prior):
    from cerberus_amd import synth
    w = synth.make_window(cfg, params=synth.default_params(n_landmarks=L, seed=seed, with_prior=prior))
    O.fill_preint(ocfg, w)
    O.solve_window(ocfg, w, O.default_opts(True, 6))
    return w


@pytest.fixture(scope="module")
def win_prior(cfg, ocfg):
    return _solved_window(cfg, ocfg, 20260927, 80, True)


@pytest.fixture(scope="module")
def win_free(cfg, ocfg):
    return _solved_window(cfg, ocfg, 20260928, 80, False)


@pytest.mark.parametrize("which,gauge", [("prior", "frame0"), ("prior", "none"), ("free", "frame0")])
def test_schur_form_equals_full_inverse(ocfg, win_prior, win_free, which, gauge):
    """Sigma_rr = 1/E + w^T Sigma_PP w / E^2 and Sigma_rP = -w^T Sigma_PP / E, with Sigma_PP the pose-system output, are the landmark rows of
    the full inverse."""
    w = win_prior if which == "prior" else win_free
    S, cols, H = lm_cov_ref.full_covariance(ocfg, w, gauge)
    _, Spp = cov_ref.outputs(S, cols)
    ix = cov_ref.camera_index(cols)
    worst_v, worst_c = 0.0, 0.0
    for l in range(w.L):
        E, wv = lm_cov_ref.pose_system_coupling(H, cols, l)
        vr, cp = lm_cov_ref.schur_form(E, wv, Spp)
        cl = cols[(9, l)].start
        worst_v = max(worst_v, abs(vr - S[cl, cl]) / S[cl, cl])
        for p in range(79):
            if ("p", p) in ix and Spp[p, p] > 0:
                worst_c = max(worst_c, abs(cp[p] - S[cl, ix[("p", p)]]) / np.sqrt(S[cl, cl] * Spp[p, p]))
    print(which, gauge, "variance %.1e  cross %.1e" % (worst_v, worst_c))
    tv, tp = lm_cov_ref.tolerances(which == "prior")
    assert worst_v < tv / 10 and worst_c < tp / 10


def test_point_jacobian_central_differences(win_prior):
    w = win_prior
    for l in (0, w.L // 2, w.L - 1):
        s = int(w.lm_start_frame[l])
        f = lm_cov_ref.first_observation(w, l)
        ps, ex, rho = w.pose[s].copy(), w.ex_pose[0].copy(), float(w.inv_depth[l])
        J = lm_cov_ref.point_jacobian(ps, ex, f, rho)
        Jn = np.zeros((3, 13))
        for c in range(13):
            h = 1e-6 * (rho if c == 12 else 1.0)
            pt = []
            for sg in (1.0, -1.0):
                d = np.zeros(13)
                d[c] = sg * h
                pt.append(lm_cov_ref.world_point(lm_cov_ref.pose_plus(ps, d[0:6]), lm_cov_ref.pose_plus(ex, d[6:12]), f, rho + d[12]))
            Jn[:, c] = (pt[0] - pt[1]) / (2 * h)
        np.testing.assert_allclose(J, Jn, rtol=1e-6, atol=1e-6 * np.abs(J).max())


def test_points_follow_the_window(win_prior):
    """points: pubPointCloud's formula with the landmark's start frame and first observation"""
    w = win_prior
    pts = lm_cov_ref.world_points(w)
    for l in (0, w.L - 1):
        s = int(w.lm_start_frame[l])
        Rs, Rc = cov_ref.quat_R(w.pose[s, 3:7]), cov_ref.quat_R(w.ex_pose[0, 3:7])
        f = w.obs[w.lm_obs_offset[l], 0:3]
        np.testing.assert_allclose(pts[l], Rs @ (Rc @ (f * (1.0 / w.inv_depth[l])) + w.ex_pose[0, :3]) + w.pose[s, :3], rtol=1e-14)


def _ulp_floor(ocfg, w, gauge, rng):
    S, cols, H = lm_cov_ref.full_covariance(ocfg, w, gauge)
    v, _, pc = lm_cov_ref.outputs(S, cols, w)
    _, _, J = cov_ref.hessian(ocfg, w)
    Jp = J * (1.0 + np.finfo(float).eps * rng.choice([-1.0, 1.0], size=J.shape))
    S2, _, _ = lm_cov_ref.full_covariance(ocfg, w, gauge, J=Jp)
    v2, _, pc2 = lm_cov_ref.outputs(S2, cols, w)
    return lm_cov_ref.errors(v2, pc2, v, pc)


def test_fp64_floor_measured(ocfg, win_prior, win_free):
    """The spread of the definition in FP64 under a one-ulp perturbation of J; the GPU tolerances stand at ten times it or more."""
    rng = np.random.default_rng(9)
    for name, w, g in (("prior", win_prior, "frame0"), ("prior", win_prior, "none"), ("no_prior", win_free, "frame0")):
        e = _ulp_floor(ocfg, w, g, rng)
        print("%-8s %-6s one-ulp J %s" % (name, g, {k: "%.1e" % v for k, v in e.items()}))
        tv, tp = lm_cov_ref.tolerances(name == "prior")
        assert 10 * e["var"] <= tv and 10 * e["pcov"] <= tp, (name, g, e)


def test_fp64_floor_against_exact(cfg, ocfg):
    """One small window: the FP64 route against the same FP64 H inverted in 40-digit arithmetic (mpmath)."""
    mp = pytest.importorskip("mpmath")
    w = _solved_window(cfg, ocfg, 4243, 24, True)
    S, cols, H = lm_cov_ref.full_covariance(ocfg, w, "frame0")
    v, _, pc = lm_cov_ref.outputs(S, cols, w)
    N = cov_ref.gauge_basis(w, cols, H.shape[0])
    with mp.workdps(40):
        A = N.T @ H @ N
        d = 1.0 / np.sqrt(np.diag(A))
        Ai = mp.inverse(mp.matrix((A * np.outer(d, d)).tolist()))
        Ae = np.array(Ai.tolist(), dtype=np.float64) * np.outer(d, d)
    ve, _, pce = lm_cov_ref.outputs(N @ Ae @ N.T, cols, w)
    e = lm_cov_ref.errors(v, pc, ve, pce)
    print("against 40 digits:", {k: "%.1e" % x for k, x in e.items()})
    assert 10 * e["var"] <= lm_cov_ref.TOL_VAR and 10 * e["pcov"] <= lm_cov_ref.TOL_PCOV, e
