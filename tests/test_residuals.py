"""CPU: the residual report's C-ABI (symbols, struct sizes, bad arguments without a device) and the definition the GPU pass is held to
(tests/resid_ref.py): its total is the oracle's window cost, and its outlier / failure flags are the reference's sets."""
import ctypes as C
import os

import numpy as np
import pytest

import resid_ref
from conftest import ROOT
from oracle import oracle_py as O
from test_covariance_gpu import _window


def test_symbols_exported():
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for n in ("vilo_batch_residuals", "vilo_window_residuals", "vilo_default_residual_opts", "vilo_last_residuals_ms"):
        assert hasattr(lib, n), n


def test_python_binding_present():
    from cerberus_amd import api
    assert callable(getattr(api.Batch, "residuals", None))
    assert callable(getattr(api.Context, "window_residuals", None))


def test_struct_sizes_match_header():
    from cerberus_amd import _ctypes as T
    assert C.sizeof(T.ResidualOpts) == 8
    assert C.sizeof(T.WindowResidual) == 136
    assert T.WindowResidual.imu_cost.offset == 16 and T.WindowResidual.visual_cost.offset == 96
    assert T.WindowResidual.n_visual_blocks.offset == 112 and T.WindowResidual.status.offset == 128
    src = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    for name in ("vilo_residual_opts", "vilo_window_residual"):
        assert "} %s;" % name in src
    assert "static_assert(sizeof(vilo_window_residual) == 136" in open(os.path.join(ROOT, "cerberus_amd", "csrc", "kernels_resid.hip")).read()


def test_bad_arguments_without_a_device():
    from cerberus_amd import api
    from cerberus_amd import _ctypes as T
    L = api.lib()
    wr = (T.WindowResidual * 1)()
    assert L.vilo_batch_residuals(None, None, None, wr, None, None, None, None, None) == -2
    assert L.vilo_window_residuals(None, 1, None, None, None, wr, None, None, None, None, None) == -2
    o = T.ResidualOpts()
    L.vilo_default_residual_opts(C.byref(o))
    assert o.outlier_threshold_px == 3.0


CASES = {
    "prior": dict(),
    "no_prior": dict(prior=False),
    "imu_only": dict(use_leg=0, leg_bias_const=1),
    "partial_F6": dict(F=6, prior=False, leg_bias_const=1),
    "td_free": dict(td_const=0),
}


@pytest.mark.parametrize("case", sorted(CASES))
@pytest.mark.parametrize("seed", [5, 6])
def test_total_is_the_oracle_window_cost(cfg, ocfg, case, seed):
    w = _window(cfg, ocfg, seed=1000 * seed + len(case), L=50, **CASES[case])
    ref = resid_ref.window_residuals(ocfg, w)
    oc = O.window_cost(ocfg, w)
    assert abs(ref["cost"] - oc) <= 1e-13 * abs(oc)
    assert ref["visual_cost"] == pytest.approx(float(ref["lm_cost"].sum()), rel=1e-15)
    assert ref["n_visual_blocks"] == int(np.isfinite(ref["obs_residuals"][:, 0]).sum() + np.isfinite(ref["obs_residuals"][:, 2]).sum())
    if not w.use_leg:
        assert not ref["imu_residuals"][:, 15:].any()
    assert not ref["imu_residuals"][w.F - 1:].any()
    assert (ref["prior_cost"] > 0) == bool(CASES[case].get("prior", True))


def test_flags_are_the_reference_sets(cfg, ocfg):
    w = _window(cfg, ocfg, seed=4242, L=60)
    chosen = [2, 11, 30, 47, 58]
    resid_ref.shift_observations(w, chosen, 10.0, cfg.focal_length)
    O.solve_window(ocfg, w, O.default_opts(True, 6))
    ref = resid_ref.window_residuals(ocfg, w)
    assert sorted(np.flatnonzero(ref["lm_flags"] & 1).tolist()) == chosen
    assert ref["n_outliers"] == len(chosen)
    assert not (ref["lm_flags"] & 2).any()
    # bit 0 is outliersRejection's test itself: (err / cnt) * FOCAL_LENGTH > 3
    for l in range(w.L):
        err, cnt = resid_ref.landmark_reprojection(w, l)
        assert bool(ref["lm_flags"][l] & 1) == (err / cnt * cfg.focal_length > 3.0)
    # bit 1 follows the sign of the inverse depth (setDepth's solve_flag = 2)
    w.inv_depth[7] = -w.inv_depth[7]
    ref = resid_ref.window_residuals(ocfg, w)
    assert np.flatnonzero(ref["lm_flags"] & 2).tolist() == [7] and ref["n_negative_depth"] == 1
