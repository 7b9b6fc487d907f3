"""CPU: the declarations of vilo_batch_trial_cost, the numpy / oracle restatement (tests/trial_ref.py) against the oracle on one window, the
floor the GPU test's oracle comparison holds ten times of, and, with the oracle alone, that the steps tests/test_trial_cost_gpu.py uses
keep every trial state's decisions clear of trouble: positive depths and no Huber block near its threshold, so that a tolerance never
hides a branch flip."""
import ctypes as C
import os

import numpy as np
import pytest

import retract_ref as RR
import trial_ref as TR
from conftest import ROOT


def _oracle_plus(X, S):
    from oracle import oracle_py as O
    return np.array([O.pose_plus(X[i], S[i]) for i in range(len(X))])


def test_declarations():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    assert C.sizeof(T.TrialRecord) == 48 and T.TRIAL_MAX_STEPS == 16
    assert (T.TRIAL_OK, T.TRIAL_NUMERIC, T.TRIAL_INVALID, T.TRIAL_NOT_FINITE) == (TR.OK, TR.NUMERIC, TR.INVALID, TR.NOT_FINITE) == (0, 1, 2, 3)
    assert tuple(f for f, _ in T.TrialRecord._fields_) == TR.FIELDS == api.TrialCost._fields[:7] == api.TrialBase._fields
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    for name in ("vilo_batch_trial_cost", "vilo_window_trial_cost", "vilo_last_trial_cost_ms", "} vilo_trial_record;",
                 "#define VILO_TRIAL_MAX_STEPS 16", "#define VILO_TRIAL_NUMERIC 1", "#define VILO_TRIAL_INVALID 2", "#define VILO_TRIAL_NOT_FINITE 3"):
        assert name in hdr, name
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for sym in ("vilo_batch_trial_cost", "vilo_window_trial_cost", "vilo_last_trial_cost_ms"):
        assert getattr(lib, sym)
    lib.vilo_last_trial_cost_ms.restype = C.c_double
    assert lib.vilo_last_trial_cost_ms(None) == -1.0
    assert lib.vilo_batch_trial_cost(None, None, 1, None, None, None, None, None, None) == -2
    assert callable(api.Batch.trial_cost) and callable(api.Context.window_trial_cost) and callable(api.window_trial_cost)


def test_trial_cost_args_checks_its_arguments():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    descs = [T.WindowDesc(), T.WindowDesc()]
    descs[0].n_landmarks, descs[1].n_landmarks = 3, 4
    K, sq, s, l, a, off = api.trial_cost_args(descs, np.zeros((2, 222)), np.zeros(7), [1, 2])
    assert (K, sq, s.shape, l.shape, a.shape, list(off)) == (1, True, (2, 1, 222), (7,), (2, 1), [0, 3, 7])
    K, sq, s, l, a, off = api.trial_cost_args(descs, np.zeros((2, 5, 222)), np.zeros(35), np.ones((2, 5)))
    assert (K, sq, a.dtype, a.flags["C_CONTIGUOUS"]) == (5, False, np.float64, True)
    for bad in (np.ones(2), np.ones((2, 4)), np.ones((5, 2))):
        with pytest.raises(ValueError, match="alpha"):
            api.trial_cost_args(descs, np.zeros((2, 5, 222)), None, bad)
    with pytest.raises(ValueError):
        api.trial_cost_args(descs, np.zeros((2, 17, 222)))


def test_trial_ref_against_the_oracle(cfg, ocfg):
    """base is the oracle's cost at x, cost_change adds up, a non-finite step is NUMERIC alone, best is the lowest cost that lowers it"""
    from oracle import oracle_py as O
    w = RR.kind_window(cfg, ocfg, "c40_ex")
    ss, _, al, bl = TR.steps([w], 3, 7)
    al[0, 1] = np.inf
    before = [a.tobytes() for a in w.state_arrays()]
    rec, base, best, states = TR.trial_cost(ocfg, w, ss[0], bl[0], al[0], _oracle_plus, parts=True)
    assert [a.tobytes() for a in w.state_arrays()] == before
    assert base["cost"] == O.window_cost(ocfg, w) and base["cost_change"] == 0.0 and base["status"] == TR.OK
    assert list(rec["status"]) == [TR.OK, TR.NUMERIC, TR.OK] and states[1] is None and np.isnan(rec["cost"][1])
    for k in (0, 2):
        t = w.twin()
        t.set_state(states[k])
        assert rec["cost"][k] == O.window_cost(ocfg, t) and rec["cost_change"][k] == base["cost"] - rec["cost"][k]
        assert rec["cost_parts"][k] == pytest.approx(rec["cost"][k], rel=TR.TRIAL_TOL)
        assert rec["visual_cost"][k] + rec["imu_cost"][k] + rec["prior_cost"][k] == pytest.approx(rec["cost"][k], rel=1e-14)
    assert best == TR.best_of(rec["status"], rec["cost"], rec["cost_change"])
    assert TR.best_of([0, 0, 1, 0], [5.0, 3.0, 1.0, 3.0], [-1.0, 1.0, 3.0, 1.0]) == 1 and TR.best_of([0, 3], [5.0, 1.0], [-1.0, 3.0]) == -1


def _batches(cfg, ocfg):
    kinds = {n: RR.kind_window(cfg, ocfg, n) for n in RR.LEG_KINDS + (RR.IMU_KIND,)}
    return [(RR.batch_of(kinds, 5), 5, 1005), (RR.batch_of(kinds, 1, (RR.IMU_KIND,)), 5, 1001)]


def test_floor_of_the_oracle_cost_in_two_orders(cfg, ocfg):
    """TR.TRIAL_MEASURED: O.window_cost against the sum of resid_ref's parts at the trial states (three per kind); ten times it is held
    here against the seed and in the GPU test against the device's order of summation."""
    worst = 0.0
    for ws, K, seed in _batches(cfg, ocfg):
        ss, _, al, bl = TR.steps(ws, K, seed)
        for i, w in enumerate(ws):
            rec = TR.trial_cost(ocfg, w, ss[i][:3], bl[i][:3], al[i][:3], _oracle_plus, parts=True)[0]
            e = float(np.abs(rec["cost_parts"] / rec["cost"] - 1).max())
            print("MEASURED window %d (F %d, L %d): two orders of summation differ by %.1e of the cost" % (i, w.F, w.L, e))
            worst = max(worst, e)
    print("MEASURED largest: %.1e (TRIAL_MEASURED %.1e)" % (worst, TR.TRIAL_MEASURED))
    assert worst <= TR.TRIAL_TOL


def test_the_gpu_tests_steps_stay_clear_of_branches(cfg, ocfg):
    """At every trial state of the W = 5, K = 5 batch and of the IMU-only window (the seeds of tests/test_trial_cost_gpu.py): every
    inverse depth positive, and no visual block's squared norm within 1e-6 relative of Huber's threshold."""
    import resid_ref
    d2 = ocfg.huber_delta ** 2
    closest = np.inf
    for ws, K, seed in _batches(cfg, ocfg):
        ss, _, al, bl = TR.steps(ws, K, seed)
        for i, w in enumerate(ws):
            for k in range(K):
                arrays, r = RR.retract(w, ss[i, k], bl[i][k], al[i, k], _oracle_plus)
                assert r["status"] == RR.OK and (arrays[5] > 0).all(), (i, k)
                t = w.twin()
                t.set_state(arrays)
                res = resid_ref.window_residuals(ocfg, t)["obs_residuals"].reshape(-1, 2)
                s2 = (res[np.isfinite(res).all(axis=1)] ** 2).sum(axis=1)
                closest = min(closest, float(np.abs(s2 / d2 - 1).min()))
    print("MEASURED closest |s2 / delta^2 - 1| over all blocks: %.2e" % closest)
    assert closest > 1e-6
