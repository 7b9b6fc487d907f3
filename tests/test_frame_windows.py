"""The windows of tests/frame_windows.py (one for every frame count from 2 to 11) test what they claim to: conditions on the INPUTS, held on
a CPU with the oracle alone, never with the code under test. A window that misses one gets another seed, landmark count or start scale in
frame_windows (and an entry in REJECTED with the measured figure), not a weaker condition."""
import ctypes as C

import numpy as np
import pytest

import const_windows as CW
import frame_windows as FR
from oracle import oracle_py as O

# what the oracle's trust-region update compares the step-quality ratio with (o_solver.cpp: min_relative_decrease; DoglegStrategy::StepAccepted)
RATIO_THRESHOLDS = (1e-3, 0.25, 0.75)
NAMES = list(FR.LEG) + list(FR.VINS)


@pytest.fixture(scope="module")
def solved(cfg, ocfg):
    """{name: (window at the oracle's state after ITERS iterations, its initial state, summary, step-quality ratio of each iteration)}.
    The oracle keeps the scalars of a solve's last iteration only (orc_last_step_scalars): iteration k's ratio is read after a solve
    of k iterations from the same start."""
    out = {}
    for name in NAMES:
        ratios = []
        for k in range(1, FR.ITERS + 1):
            w = FR.make(cfg, ocfg, name)
            init = w.clone_state()
            s = O.solve_window(ocfg, w, O.default_opts(True, k))
            g = (C.c_double * 12)()
            O.lib().orc_last_step_scalars(g)
            ratios.append(float(g[5]))
        out[name] = (w, init, s, ratios)
        ct = np.array(s.cost_trace[:s.iterations + 1])
        print("MEASURED frame window %-10s F %2d, %2d landmarks, mask LB %d EX %d TD %d: cost %.6g, relative decrease per step %s; step-quality ratios %s"
              % ((name, w.F, w.L) + tuple(int(c) for c in CW.mask_of(w)) + (ct[0], " ".join("%.2e" % d for d in -np.diff(ct) / ct[:-1]),
                 " ".join("%.3f" % r for r in ratios))))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_constant_blocks_stay_put(solved, name):
    w, init, _, _ = solved[name]
    const = CW.constant_arrays(w)
    assert 2 in const and 4 in const and (3 in const) == (not name.endswith("_exfree")), (name, const)
    for i in const:
        np.testing.assert_array_equal(w.state_arrays()[i], init[i])
    if 3 not in const:   # and a free block moves: the flag is what holds the others
        assert np.abs(w.ex_pose - init[3]).max() > 0, name
    for i in (0, 1):     # the frames that are there move, the absent ones are not the oracle's to touch
        assert np.abs(w.state_arrays()[i][:w.F] - init[i][:w.F]).max() > 0, (name, i)
        np.testing.assert_array_equal(w.state_arrays()[i][w.F:], init[i][w.F:])


@pytest.mark.parametrize("name", NAMES)
def test_decisions_sit_away_from_thresholds(solved, name):
    """Every iteration a successful step, the cost falling at every one by MIN_DECREASE of itself or more, and no step-quality ratio within 10 % of a value the trust-region
    update compares it with: the GPU's equal-decisions assertion does not turn on rounding."""
    _, _, s, ratios = solved[name]
    assert (s.iterations, s.num_successful) == (FR.ITERS, FR.ITERS), name
    ct = np.array(s.cost_trace[:s.iterations + 1])
    assert (np.diff(ct) < 0).all(), (name, ct)
    assert (-np.diff(ct) >= FR.MIN_DECREASE * ct[:-1]).all(), (name, -np.diff(ct) / ct[:-1])
    assert len(ratios) == FR.ITERS
    for r in ratios:
        for t in RATIO_THRESHOLDS:
            assert abs(r - t) > 0.1 * t, (name, r, t)


@pytest.mark.parametrize("name", NAMES)
def test_oracle_solve_is_repeatable(cfg, ocfg, solved, name):
    w = FR.make(cfg, ocfg, name)
    s = O.solve_window(ocfg, w, O.default_opts(True, FR.ITERS))
    assert s.final_cost == solved[name][2].final_cost
    assert list(s.cost_trace[:s.iterations + 1]) == list(solved[name][2].cost_trace[:s.iterations + 1])
    for x, y in zip(w.state_arrays(), solved[name][0].state_arrays()):
        np.testing.assert_array_equal(x, y)


def test_the_set_has_the_intended_shape(cfg, ocfg):
    S, V = FR.leg_set(cfg, ocfg), FR.vins_set(cfg, ocfg)
    # one default-mask leg window for every frame count, the field-shaped and the free-extrinsics variants, the IMU-only counts
    assert [S["g%d" % F].F for F in range(2, 12)] == list(range(2, 12))
    assert [S["g%d_field" % F].F for F in (3, 6, 10)] == [3, 6, 10] and [S["g%d_exfree" % F].F for F in (5, 7, 10)] == [5, 7, 10]
    assert sorted(w.F for w in V.values()) == [2, 3, 5, 6, 7, 9, 10]
    assert not FR.REJECTED or all(len(r) == 4 for r in FR.REJECTED)
    for name, w in list(S.items()) + list(V.items()):
        assert w.prior.struct.valid == 0 and 8 <= w.L <= 60, (name, w.L)
        assert CW.mask_of(w) == (True, not name.endswith("_exfree"), True), name
        assert w.use_leg == (0 if name in V else 1) and w.leg_bias_const == 1
        # every start frame from 0 to F - 2 has a landmark, none starts later (at F = 2: frame 0 alone), every track fits the window
        assert sorted(set(w.lm_start_frame.tolist())) == list(range(w.F - 1)), name
        K = np.diff(w.lm_obs_offset)
        assert (K >= 2).all() and (w.lm_start_frame + K <= w.F).all() and w.n_obs == K.sum() == len(w.obs), name
        assert (K == w.F - w.lm_start_frame).all() == (not name.endswith("_field")), name
    for F in (3, 6, 10):   # ragged, part mono (at F = 3 a track has 2 or 3 observations)
        w = S["g%d_field" % F]
        assert w.obs_is_stereo.mean() < 0.9 and len(set(np.diff(w.lm_obs_offset).tolist())) > 1, F
    # the batches: every aligned group of four holds four frame counts; 2 frames beside 11 and 10; each window at two positions of the
    # leg batch of 32 (16 windows), at three or more from 48 on, and of the IMU-only batches
    for Sx, W, least in ((S, 32, 2), (S, 48, 3), (S, 257, 3), (V, 32, 3)):
        ws, names = FR.batch_of(Sx, W)
        assert len(ws) == W and len({id(w) for w in ws}) == W and len({id(w.pose) for w in ws}) == W
        Fs = [w.F for w in ws]
        for p, (w, nm) in enumerate(zip(ws, names)):
            assert w.F == Sx[nm].F and CW.mask_of(w) == CW.mask_of(Sx[nm]) and w.obs is Sx[nm].obs, (p, nm)
        for g in range(0, W - 3, 4):
            assert len(set(Fs[g:g + 4])) == 4, (W, g, Fs[g:g + 4])
        assert set(names) == set(Sx) and all(names.count(nm) >= least for nm in Sx), W
        groups = [tuple(Fs[g:g + 4]) for g in range(0, W - 3, 4)]
        if Sx is S:
            assert (2, 11, 3, 10) in groups and (10, 2, 9, 3) in groups
        else:
            assert Fs[:4] == [2, 10, 3, 9]
