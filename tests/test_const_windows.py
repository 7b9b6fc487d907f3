"""The windows of tests/const_windows.py test what they claim to: conditions on the INPUTS, held on a CPU with the oracle alone, never with
the code under test. A window that misses one gets another seed or a larger start perturbation of the block in question in
const_windows (and an entry in REJECTED_SEEDS), not a weaker condition."""
import ctypes as C

import numpy as np
import pytest

import const_windows as CW
import field_windows as FW
from oracle import oracle_py as O
from test_kernel_paths import _rel_states

NEED = 1000.0 * 1e-8   # a flag moves the oracle's answer by 1000 times the 1e-8 the kernel forms are held to (tests/test_alt_config.py's margin)
# what the oracle's trust-region update compares the step-quality ratio with (o_solver.cpp: min_relative_decrease; DoglegStrategy::StepAccepted)
RATIO_THRESHOLDS = (1e-3, 0.25, 0.75)
NAMES = list(CW.LEG) + list(CW.VINS)


def _make(cfg, ocfg, name, priors):
    return CW.leg_window(cfg, ocfg, name) if name in CW.LEG else CW.vins_window(cfg, ocfg, name, priors)


@pytest.fixture(scope="module")
def solved(cfg, ocfg):
    """{name: (window at the oracle's state after ITERS iterations, its initial state, summary, step-quality ratio of each iteration)}.
    The oracle keeps the scalars of a solve's last iteration only (orc_last_step_scalars): iteration k's ratio is read after a solve
    of k iterations from the same start."""
    priors, out = {}, {}
    for name in NAMES:
        ratios = []
        for k in range(1, CW.ITERS + 1):
            w = _make(cfg, ocfg, name, priors)
            init = w.clone_state()
            s = O.solve_window(ocfg, w, O.default_opts(True, k))
            g = (C.c_double * 12)()
            O.lib().orc_last_step_scalars(g)
            ratios.append(float(g[5]))
        out[name] = (w, init, s, ratios)
        print("MEASURED const window %-13s mask LB %d EX %d TD %d: cost trace %s; step-quality ratios %s"
              % ((name,) + tuple(int(c) for c in CW.mask_of(w)) + (" ".join("%.4g" % c for c in s.cost_trace[:s.iterations + 1]),
                 " ".join("%.3f" % r for r in ratios))))
    return out


FLAG_PAIRS = [("c40_ex", "c40_free"), ("c40_lb", "c40_free"), ("c40_ex_lb", "c40_free"), ("c40_ex", "c40_lb"), ("c40_ex", "c40_ex_lb"),
              ("c40_lb", "c40_ex_lb"), ("v40_ex", "v40")]


@pytest.mark.parametrize("a,b", FLAG_PAIRS)
def test_flags_move_the_answer(solved, a, b):
    """Same generator seed, same start state, another mask: the oracle's states after ITERS iterations differ by 1000 bounds or more.
    Measured: ex_const 5e-2, leg_bias_const 7e-3, both 5e-2 against the control; 5e-3 .. 5e-2 among themselves; IMU-only ex_const 0.27."""
    wa, ia, _, _ = solved[a]
    wb, ib, _, _ = solved[b]
    for x, y in zip(ia, ib):
        np.testing.assert_array_equal(x, y)   # (the same window but for the flags)
    e = _rel_states(wa.state_arrays(), wb.state_arrays())
    print("MEASURED flag effect %s against %s: %.3e" % (a, b, e))
    assert e >= NEED, (a, b, e)


@pytest.mark.parametrize("name", NAMES)
def test_constant_blocks_stay_put(solved, name):
    w, init, _, _ = solved[name]
    const = CW.constant_arrays(w)
    assert 2 in const or (w.use_leg and not w.leg_bias_const)
    for i in const:
        np.testing.assert_array_equal(w.state_arrays()[i], init[i])
    for i in (2, 3, 4):   # and a free block moves: the flag is what holds the others
        if i not in const:
            assert np.abs(w.state_arrays()[i][:w.F] - init[i][:w.F]).max() > 0, (name, i)


@pytest.mark.parametrize("name", NAMES)
def test_decisions_sit_away_from_thresholds(solved, name):
    """Every iteration a successful step, the cost never rising, and no step-quality ratio within 10 % of a value the trust-region update
    compares it with: the GPU's equal-decisions assertion does not turn on rounding."""
    _, _, s, ratios = solved[name]
    assert (s.iterations, s.num_successful) == (CW.ITERS, CW.ITERS), name
    ct = np.array(s.cost_trace[:s.iterations + 1])
    assert (np.diff(ct) < 0).all(), (name, ct)
    for r in ratios:
        for t in RATIO_THRESHOLDS:
            assert abs(r - t) > 0.1 * t, (name, r, t)
        assert r > 0.75   # (so each step also widens the radius: one branch of StepAccepted for the whole set)


def test_oracle_solve_is_repeatable(cfg, ocfg, solved):
    for name in ("c40_ex_lb", "v40"):
        w = _make(cfg, ocfg, name, {})
        s = O.solve_window(ocfg, w, O.default_opts(True, CW.ITERS))
        assert s.final_cost == solved[name][2].final_cost
        for x, y in zip(w.state_arrays(), solved[name][0].state_arrays()):
            np.testing.assert_array_equal(x, y)


def test_the_set_has_the_intended_shape(cfg, ocfg):
    S, V = CW.const_set(cfg, ocfg), CW.vins_set(cfg, ocfg)
    # c200_ex: the bench's size, ragged groups, part mono
    w = S["c200_ex"]
    assert w.L == 200 and w.prior.struct.valid == 1 and len(FW.ragged_groups(w)) >= 3
    assert 0.15 < 1.0 - w.obs_is_stereo.mean() < 0.35
    # the four c40 windows: one generator seed, one start state, a prior each
    for n in ("c40_ex", "c40_lb", "c40_ex_lb"):
        for x, y in zip(S[n].state_arrays(), S["c40_free"].state_arrays()):
            np.testing.assert_array_equal(x, y)
        np.testing.assert_array_equal(S[n].obs, S["c40_free"].obs)
        assert S[n].prior.struct.valid == 1 and S[n].F == 11
    # the extrinsics start off the calibration the observations were generated with
    assert np.abs(S["c40_ex"].ex_pose[:, :3] - np.array([[0.10076, 0.025, 0.1114], [0.10076, -0.025, 0.1114]])).max() > 1e-3
    # partial windows: no prior, the mask optimization() gives frame_count < WINDOW_SIZE
    for n, F in (("c60_partial8", 8), ("c60_partial4", 4)):
        assert S[n].F == F and S[n].prior.struct.valid == 0 and CW.mask_of(S[n]) == (True, True, True) and S[n].L >= 8
    assert V["v60_partial8"].F == 8 and V["v60_partial8"].prior.struct.valid == 0 and V["v130_noprior"].prior.struct.valid == 0
    # the IMU-only prior: the block table of an IMU-only marginalisation (poses 0 .. 9, speed / biases of frame 0, extrinsics, td)
    for n in ("v40", "v40_ex", "v40_skip", "v40_td"):
        p = V[n].prior
        ids = [b[0] for b in p.blocks()]
        assert p.struct.valid == 1 and ids == list(range(10)) + [16, 48, 49, 64] and p.n == 82, (n, ids)
        assert not any(i >> 4 == 2 for i in ids)                                   # no leg-bias block
        idx = {b[0]: b[2] for b in p.blocks()}
        assert idx[16] - idx[0] == 60 and idx[48] - idx[16] == 9                   # frame 0: 6 + 9 = 15 dimensions, extrinsics next
    assert S["c40_free"].prior.n == 86                                             # (the generator's: with the leg-bias block)
    for n, w in V.items():
        assert w.use_leg == 0 and w.leg_bias_const == 1, n
    assert V["v40_skip"].preint[4, 0] == V["v40_skip"].preint_imu[4, 0] == 11.0
    np.testing.assert_array_equal(V["v40"].pose, V["v40_ex"].pose)
    # every mask of the set is in a batch of 32, different masks side by side, each window at three positions or more
    for Sx, td_name, masks in ((S, "c40_ex_td", {(False, False, True), (False, True, True), (True, False, True), (True, True, True), (False, True, False)}),
                               (V, "v40_td", {(True, False, True), (True, True, True), (True, False, False)})):
        for with_td in (False, True):
            ws, names = CW.batch_of(Sx, 32, with_td)
            assert len(ws) == 32 and len({id(w) for w in ws}) == 32 and len({id(w.pose) for w in ws}) == 32
            got = {CW.mask_of(w) for w in ws}
            assert got == (masks if with_td else {m for m in masks if m[2]}), got
            assert (names[CW.TD_POSITION] == td_name) == with_td and names.count(td_name) == int(with_td)
            for nm in set(names) - {td_name}:
                assert names.count(nm) >= 3, nm
            assert sum(CW.mask_of(a) != CW.mask_of(b) for a, b in zip(ws, ws[1:])) >= 16
            for w, nm in zip(ws, names):
                assert CW.mask_of(w) == CW.mask_of(Sx[nm])
