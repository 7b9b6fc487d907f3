"""The windows of tests/field_windows.py have the properties the GPU tests on them rely on: conditions on the INPUTS, held on a CPU with
the oracle, tests/resid_ref.py and the restated packing of tests/test_batch_pack.py alone, never with the code under test. A window that
misses one is changed in field_windows.RECIPES (seed, outlier share or size), not the condition."""
import numpy as np
import pytest

import field_windows as FW
import resid_ref
from oracle import oracle_py as O
from test_batch_pack import restate

NAMES = list(FW.RECIPES)


@pytest.fixture(scope="module")
def solved(cfg, ocfg):
    """{name: (window as handed over, window at the oracle's state after ITERS iterations, its summary, a second run's summary)}"""
    out = {}
    for name in NAMES:
        w0 = FW.field_window(cfg, ocfg, name)
        runs = []
        for _ in range(2):
            w = FW.field_window(cfg, ocfg, name)
            runs.append((w, O.solve_window(ocfg, w, O.default_opts(True, FW.ITERS))))
        out[name] = (w0, runs[0][0], runs[0][1], runs[1][1], runs[1][0])
    return out


def _lane_lengths(w):
    """Per packed wave, the track lengths of its occupied lanes, from the flag image DESIGN 3 lays out (test_batch_pack.restate)."""
    t = w.twin()   # (a partial window keeps 11-frame state arrays; the restatement takes F rows)
    t.pose, t.speed_bias, t.leg_bias = w.pose[:w.F], w.speed_bias[:w.F], w.leg_bias[:w.F]
    r = restate([t])
    waves = r["waves"].reshape(-1, 14).astype(int)
    out = []
    for v in waves:
        lanes, kmax, flag_off = v[2], v[3], v[13]
        fl = r["flags"][flag_off:flag_off + kmax * lanes].reshape(kmax, lanes)
        k = (fl != 0).sum(axis=0)
        out.append(k[k > 0])
    return out


@pytest.mark.parametrize("name", NAMES)
def test_wave_structure(solved, name):
    w = solved[name][0]
    lanes = _lane_lengths(w)
    assert sum(len(k) for k in lanes) == w.L
    ragged = [k for k in lanes if len(set(k.tolist())) > 1]
    assert ragged, name
    # by construction: in the largest start-frame group a full-length track next to one of two observations
    K = np.diff(w.lm_obs_offset)
    s = int(np.argmax(np.bincount(w.lm_start_frame)))
    members = np.flatnonzero(w.lm_start_frame == s)
    assert K[members[0]] == w.F - s > 2 and K[members[1]] == 2
    assert s in FW.ragged_groups(w)   # (the plain comparison the GPU tests use sees it too)
    if name == "f70_chunks":
        assert (w.lm_start_frame == 0).sum() == 70 > 64 and len(lanes) == 2 and all(len(set(k.tolist())) > 1 for k in lanes)
    if name == "f200":
        groups = np.bincount(w.lm_start_frame)
        assert (groups > 1).sum() >= 3


@pytest.mark.parametrize("name", NAMES)
def test_factor_coverage(solved, ocfg, name):
    w = solved[name][0]
    K = np.diff(w.lm_obs_offset)
    assert K.min() >= 2 and (K <= w.F - w.lm_start_frame).all()
    fc = FW.factor_counts(w)
    assert (fc >= 1).all() and (fc == 1).sum() >= 1, name
    one = np.flatnonzero(fc == 1)[0]
    o0 = w.lm_obs_offset[one]
    assert K[one] == 2 and not w.obs_is_stereo[o0:o0 + 2].any()
    # the numpy definition counts the same factors
    assert resid_ref.window_residuals(ocfg, w)["n_visual_blocks"] == fc.sum()
    first = w.obs_is_stereo[w.lm_obs_offset[:-1]]
    later = np.delete(w.obs_is_stereo, w.lm_obs_offset[:-1])
    assert (first == 0).any() and (later == 0).any()
    if name == "f40_allmono":
        assert not w.obs_is_stereo.any()
    else:
        assert (first != 0).any() and (later != 0).any()
        share = 1.0 - w.obs_is_stereo.mean()
        assert 0.15 < share < 0.35, share


@pytest.mark.parametrize("name", NAMES)
def test_huber_activity_at_the_oracles_state(solved, ocfg, name):
    w = solved[name][1]
    r = resid_ref.window_residuals(ocfg, w)
    active = r["n_huber_active"] / r["n_visual_blocks"]
    print("MEASURED field window %s: %d visual factors, %.1f %% on the Huber branch after %d oracle iterations" % (name, r["n_visual_blocks"], 100 * active, FW.ITERS))
    assert active >= 0.03, (name, active)
    assert 1.0 - active >= 0.5, (name, active)


@pytest.mark.parametrize("name", NAMES)
def test_reprojection_errors_are_resolved_by_fp64(solved, ocfg, name):
    """A landmark's mean reprojection error (Estimator::reprojectionError) is a difference of image coordinates of magnitude up to 1: one
    ulp of a coordinate (1.1e-16) is 1e-12 of an error of 0.05 px / 460. From 0.1 px on, the 1e-12 relative bound of the residual tests
    asks for the last two ulps, not for less than one — at the state handed over and at the oracle's after ITERS iterations."""
    for w in solved[name][:2]:
        px = resid_ref.window_residuals(ocfg, w)["lm_reproj_px"]
        assert px.min() >= 0.1, (name, float(px.min()))


def _reprojection_regrouped(Ri, Pi, rici, tici, Rj, Pj, ricj, ticj, depth, uvi, uvj):
    """resid_ref.reprojection_error with the same products grouped another way: equal in exact arithmetic."""
    pts_w = (Ri @ rici) @ (depth * uvi) + (Ri @ tici + Pi)
    pts_cj = (Rj @ ricj).T @ (pts_w - Pj) - ricj.T @ ticj
    r = np.array([pts_cj[0] / pts_cj[2] - uvj[0], pts_cj[1] / pts_cj[2] - uvj[1]])
    return np.sqrt(r @ r)


def _reproj_px_two_ways(cfg, w, monkeypatch):
    out = []
    for fn in (resid_ref.reprojection_error, _reprojection_regrouped):
        monkeypatch.setattr(resid_ref, "reprojection_error", fn)
        ec = [resid_ref.landmark_reprojection(w, l) for l in range(w.L)]
        out.append(np.array([e / c * cfg.focal_length for e, c in ec]))
    monkeypatch.undo()
    return out


@pytest.mark.parametrize("name", NAMES)
def test_two_groupings_of_the_reprojection_sum_agree_from_a_tenth_of_a_pixel_on(solved, cfg, name, monkeypatch):
    """What the 0.1 px condition buys, with numpy alone: on every landmark of the set, at both states, two groupings of the transcribed
    sum agree within the residual tests' 1e-12 (measured: at most 3e-13)."""
    for w in solved[name][:2]:
        a, b = _reproj_px_two_ways(cfg, w, monkeypatch)
        assert a.min() >= 0.1 and (np.abs(a - b) / a).max() < 1e-12, (name, float((np.abs(a - b) / a).max()))


@pytest.mark.parametrize("name", sorted(FW.REJECTED_SHAPER_SEEDS))
def test_below_a_tenth_of_a_pixel_two_groupings_differ_by_more_than_the_bound(cfg, ocfg, name, monkeypatch):
    """Why the shaper seeds tried first were not kept: the oracle's solve leaves a landmark under 0.1 px (0.034 px and 0.004 px), and on
    it the two groupings, both numpy, both FP64, differ by more than 1e-12 of the error (1.5e-12 and 1.9e-12) while they agree within it on
    every landmark from 0.1 px on. No evaluation can be held to 1e-12 of a reference that its own regrouping moves by more."""
    w = FW.field_window(cfg, ocfg, name, shaper_seed=FW.REJECTED_SHAPER_SEEDS[name])
    O.solve_window(ocfg, w, O.default_opts(True, FW.ITERS))
    a, b = _reproj_px_two_ways(cfg, w, monkeypatch)
    rel = np.abs(a - b) / a
    small = a < 0.1
    print("MEASURED %s, shaper seed %d: smallest error %.4f px, groupings differ by %.2e there, by at most %.2e from 0.1 px on"
          % (name, FW.REJECTED_SHAPER_SEEDS[name], a.min(), rel[small].max(), rel[~small].max()))
    assert small.sum() >= 1 and rel[small].max() > 1e-12
    assert rel[~small].max() < 1e-12


@pytest.mark.parametrize("name", NAMES)
def test_oracle_solve_is_repeatable(solved, name):
    _, wa, a, b, wb = solved[name]
    assert (a.iterations, a.num_successful) == (b.iterations, b.num_successful)
    assert a.iterations == FW.ITERS and a.num_successful >= 1
    assert a.final_cost == b.final_cost
    for x, y in zip(wa.state_arrays(), wb.state_arrays()):
        np.testing.assert_array_equal(x, y)


@pytest.mark.parametrize("kw", [dict(), dict(mono=1.0), dict(outlier=0.5, min_obs=3)])
def test_the_shaper_keeps_what_it_does_not_shape(cfg, ocfg, kw):
    a, b = FW._filled(cfg, ocfg, 40, 7), FW._filled(cfg, ocfg, 40, 7)
    full, short, one = FW.field_shape(b, 3, **kw)
    assert (a.L, a.F) == (b.L, b.F)
    np.testing.assert_array_equal(a.lm_start_frame, b.lm_start_frame)
    for x, y in zip(a.state_arrays(), b.state_arrays()):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(a.preint, b.preint)
    np.testing.assert_array_equal(a.preint_imu, b.preint_imu)
    assert a.prior.blocks() == b.prior.blocks() and a.prior.n == b.prior.n
    assert a.prior.struct.valid == b.prior.struct.valid == 1
    for x, y in ((a.prior.x0, b.prior.x0), (a.prior.J0, b.prior.J0), (a.prior.r0, b.prior.r0)):
        np.testing.assert_array_equal(x, y)
    Ka, Kb = np.diff(a.lm_obs_offset), np.diff(b.lm_obs_offset)
    assert b.n_obs == Kb.sum() == len(b.obs) == len(b.obs_is_stereo) and b.lm_obs_offset[0] == 0
    free = np.setdiff1d(np.arange(a.L), [full, short, one])
    assert (Kb[free] >= kw.get("min_obs", 2)).all() and (Kb <= Ka).all()
    assert Kb[full] == Ka[full] and Kb[short] == 2 and Kb[one] == 2 and a.lm_start_frame[full] == a.lm_start_frame[short]
    # every kept observation is the generator's but for the outliers' image points; velocities and td untouched
    for l in range(a.L):
        oa, ob = a.obs[a.lm_obs_offset[l]:a.lm_obs_offset[l] + Kb[l]], b.obs[b.lm_obs_offset[l]:b.lm_obs_offset[l + 1]]
        np.testing.assert_array_equal(oa[:, [2, 5, 6, 7, 8, 9, 10]], ob[:, [2, 5, 6, 7, 8, 9, 10]])
    moved = np.concatenate([np.abs(a.obs[a.lm_obs_offset[l]:a.lm_obs_offset[l] + Kb[l]] - b.obs[b.lm_obs_offset[l]:b.lm_obs_offset[l + 1]]).max(axis=1)
                            for l in range(a.L)]) > 0
    assert abs(moved.mean() - kw.get("outlier", 0.05)) < 0.08
    # a second call with the same seed gives the same window
    c = FW._filled(cfg, ocfg, 40, 7)
    FW.field_shape(c, 3, **kw)
    np.testing.assert_array_equal(b.obs, c.obs); np.testing.assert_array_equal(b.obs_is_stereo, c.obs_is_stereo)
    np.testing.assert_array_equal(b.lm_obs_offset, c.lm_obs_offset)
