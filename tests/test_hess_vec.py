"""CPU: the Hessian-vector call's C-ABI (symbols, struct size, argument checks without a device) and the definition the GPU pass is held to
(tests/hv_ref.py): symmetry and positive semi-definiteness, H e_i against diag(H), the FP64 floor of the definition (one-ulp-moved
states; the oracle's classes against the compiled reference's) and the non-zero denominators of the test vectors. Measured figures are
printed; hv_ref.FLOOR / FLOOR_VHV / FLOOR_GV / FLOOR_GV_SOLVED_SAME_BITS stand above them."""
import ctypes as C
import os

import numpy as np
import pytest

import grad_ref
import hv_ref
from conftest import ROOT
from oracle import oracle_py as O
from oracle import ref_py as R
from test_covariance_gpu import _window
from test_gn_step import _ref, _ulp_moved


def test_symbols_exported():
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for n in ("vilo_batch_hessian_vector", "vilo_window_hessian_vector", "vilo_last_hess_vec_ms"):
        assert hasattr(lib, n), n


def test_python_binding_present():
    from cerberus_amd import api
    assert callable(getattr(api.Batch, "hessian_vector", None))
    assert callable(getattr(api.Context, "window_hessian_vector", None))
    assert api.HessianVector._fields == ("state_out", "lm_out", "offsets", "n_vec", "vHv", "g_dot_v", "model_cost_change", "status")


def test_struct_size_matches_header():
    from cerberus_amd import _ctypes as T
    assert C.sizeof(T.HessVecRecord) == 32 and T.HessVecRecord.status.offset == 24 and T.HV_MAX_VECTORS == 16
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    assert "} vilo_hess_vec_record;" in hdr and "#define VILO_HV_MAX_VECTORS 16" in hdr
    src = open(os.path.join(ROOT, "cerberus_amd", "csrc", "kernels_hessvec.hip")).read()
    assert "static_assert(sizeof(vilo_hess_vec_record) == 32" in src


def test_bad_arguments_without_a_device():
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    L = api.lib()
    rec = (T.HessVecRecord * 1)()
    assert L.vilo_batch_hessian_vector(None, None, 1, None, None, rec, None, None) == -2
    assert L.vilo_window_hessian_vector(None, 1, None, None, 1, None, None, rec, None, None) == -2
    assert L.vilo_last_hess_vec_ms(None) == -1.0


def test_hess_vec_args_validation():
    from cerberus_amd import api

    class D:
        def __init__(self, n):
            self.n_landmarks = n
    descs = [D(3), D(5)]
    K, sq, sv, lv, off = api.hess_vec_args(descs, np.zeros((2, 222)))
    assert (K, sq, sv.shape, lv) == (1, True, (2, 1, 222), None) and off.tolist() == [0, 3, 8]
    K, sq, sv, lv, off = api.hess_vec_args(descs, np.zeros((2, 4, 222)), np.zeros(32))
    assert (K, sq, lv.shape) == (4, False, (32,)) and sv.flags.c_contiguous
    assert api.hess_vec_args(descs, None, np.zeros(24))[:2] == (3, False)
    assert api.hess_vec_args(descs, None, np.zeros(8))[:2] == (1, True)
    lm = np.arange(24.0)
    assert api.hess_vec_lm_block(lm, off, 3, 1).tolist() == lm[9:].reshape(3, 5).tolist()
    for bad in (dict(), dict(state_vec=np.zeros((3, 222))), dict(state_vec=np.zeros((2, 221))), dict(state_vec=np.zeros((2, 17, 222))),
                dict(state_vec=np.zeros((2, 2, 222)), lm_vec=np.zeros(8)), dict(lm_vec=np.zeros(9)), dict(lm_vec=np.zeros((2, 8))),
                dict(state_vec=np.zeros((2, 0, 222)))):
        with pytest.raises(ValueError):
            api.hess_vec_args(descs, **bad)


# ---- the definition ----
FLOOR_CASES = [(L, prior) for L in (40, 120) for prior in (True, False)]


def test_reference_is_symmetric_and_positive_semidefinite(cfg, ocfg):
    w = _window(cfg, ocfg, seed=601, L=40)
    sy = hv_ref.system(ocfg, w)
    vs = hv_ref.test_vectors(sy, 1)
    u, v = vs["random"], vs["random_plain"]
    a, b = float(u @ hv_ref.hess_vec(sy, v)), float(v @ hv_ref.hess_vec(sy, u))
    den = float(np.abs(u) @ hv_ref.bound(sy, v))
    print("MEASURED symmetry of the reference: |u.Hv - v.Hu| = %.1e of |u|.|H||v|" % (abs(a - b) / den))
    assert abs(a - b) <= 1e-14 * den
    for name, x in vs.items():
        vhv, gv, m = hv_ref.record(sy, x)
        assert vhv >= 0.0 and m == -gv - 0.5 * vhv, name
        assert abs(vhv - float(x @ hv_ref.hess_vec(sy, x))) <= 1e-13 * float(np.abs(x) @ hv_ref.bound(sy, x)), name
    # the Cauchy point of the quadratic model decreases it
    vhv, gv, m = hv_ref.record(sy, vs["minus_g"])
    alpha = -gv / vhv
    assert alpha > 0 and hv_ref.record(sy, alpha * vs["minus_g"])[2] > 0.0


def test_unit_vectors_reproduce_the_diagonal(cfg, ocfg):
    for kw in (dict(), dict(prior=False, F=5, leg_bias_const=1)):
        w = _window(cfg, ocfg, seed=602, L=40, **kw)
        sy = hv_ref.system(ocfg, w)
        h = (sy["J"] ** 2).sum(axis=0)
        n = sy["J"].shape[1]
        for i in range(0, n, 7):
            e = np.zeros(n)
            e[i] = 1.0
            assert abs(hv_ref.hess_vec(sy, e)[i] - h[i]) <= 1e-14 * h[i]
            s, lm = hv_ref.arrays(sy, e, w.L)
            assert hv_ref.columns(sy, s, lm).tolist() == e.tolist()
        assert int(grad_ref.free_mask(w).sum()) + w.L == n


def test_vectors_have_nonzero_denominators(cfg, ocfg):
    for L, prior in FLOOR_CASES:
        w = _window(cfg, ocfg, seed=901 + L + int(prior), L=L, prior=prior)
        sy = hv_ref.system(ocfg, w)
        for name, v in hv_ref.test_vectors(sy, 7, unit=False).items():
            assert (hv_ref.bound(sy, v) > 0.0).all(), (L, prior, name)


def test_fp64_floor_measured(cfg, ocfg):
    """The spread of the definition in FP64, as DESIGN 4.16 and 4.27 measured theirs: every state entry moved by one unit in the last
    place (seeded signs), and the oracle's classes against the compiled reference's (where built), in the metric of the GPU test:
    windows of 40 and 120 landmarks, with and without a prior, at the initial and a solved state; the vectors of the GPU test."""
    rng = np.random.default_rng(12)
    fl, fv, fg, same_bits = 0.0, 0.0, {c: 0.0 for c in hv_ref.FLOOR_GV}, 0.0
    for L, prior in FLOOR_CASES:
        for solved in (False, True):
            w = _window(cfg, ocfg, seed=901 + L + int(prior), L=L, prior=prior)
            if solved:
                O.solve_window(ocfg, w, O.default_opts(True, 6))
            with _ref():
                a = hv_ref.system(ocfg, w)
                m = hv_ref.system(ocfg, _ulp_moved(w, rng))
            o = hv_ref.system(ocfg, w) if R.available() else a
            worst = np.zeros((2, 3))
            for name, v in hv_ref.test_vectors(a, 7).items():
                for i, other in enumerate((m, o)):
                    e = hv_ref.error(a, hv_ref.hess_vec(other, v), v)
                    vhv, gv, _ = hv_ref.record(other, v)
                    assert np.isfinite(e), (L, prior, solved, name)
                    worst[i] = np.maximum(worst[i], (e,) + hv_ref.scalar_errors(a, v, vhv, gv))
            print("MEASURED floor, L %3d prior %d solved %d: product one ulp %.1e oracle/reference %.1e; vHv one ulp %.1e oracle/reference %.1e; "
                  "g.v one ulp %.1e oracle/reference %.1e" % (L, prior, solved, worst[0, 0], worst[1, 0], worst[0, 1], worst[1, 1], worst[0, 2], worst[1, 2]))
            cls = "solved" if solved else "initial"
            fl, fv, fg[cls] = max(fl, worst[:, 0].max()), max(fv, worst[:, 1].max()), max(fg[cls], worst[:, 2].max())
            if solved:
                same_bits = max(same_bits, worst[1, 2])
    print("MEASURED floor (%s): product %.1e (FLOOR %.0e, TOL %.0e); vHv %.1e (FLOOR_VHV %.0e); g.v per class %s (FLOOR_GV %s)"
          % ("one-ulp move and the oracle against the compiled reference" if R.available() else
             "the compiled reference is not built: the one-ulp move of the oracle alone, the oracle/reference figures are 0 by construction",
             fl, hv_ref.FLOOR, hv_ref.TOL, fv, hv_ref.FLOOR_VHV, {c: "%.1e" % x for c, x in fg.items()}, hv_ref.FLOOR_GV))
    assert fl <= hv_ref.FLOOR and fv <= hv_ref.FLOOR_VHV
    for c, x in fg.items():
        assert x <= hv_ref.FLOOR_GV[c], (c, x)
    print("MEASURED floor: g.v at a solved state, the oracle against the compiled reference at the same bits: %.1e (FLOOR_GV_SOLVED_SAME_BITS %.0e)"
          % (same_bits, hv_ref.FLOOR_GV_SOLVED_SAME_BITS))
    assert same_bits <= hv_ref.FLOOR_GV_SOLVED_SAME_BITS
