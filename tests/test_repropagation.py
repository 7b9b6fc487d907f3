"""BASELINE configs[2]: "K1 re-propagation of all 10 intervals inside the iteration". With the samples of a window's intervals at hand,
every IMULegFactor evaluation integrates its interval again (IMULegIntegrationBase::repropagate, imu_leg_integration_base.cpp:62-86)
at the biases of the evaluation point — in the oracle through orc_set_repropagation, on the device through vilo_batch_set_samples."""
import numpy as np
import pytest

from oracle import oracle_py as O


def _window(cfg, ocfg, **kw):
    from cerberus_amd import synth
    w = synth.make_window(cfg, params=synth.default_params(config=3, **kw))
    O.fill_preint(ocfg, w)
    return w


def test_400hz_window_shape(cfg, ocfg):
    """27 samples per interval (26 x 2.5 ms + one trimmed step) plus the constructor sample."""
    w = _window(cfg, ocfg, n_landmarks=30, seed=3)
    n = np.diff(w.sample_offsets)
    assert n.shape == (10,) and np.all(n == 28)
    dt = w.samples[w.sample_offsets[0] + 1: w.sample_offsets[1], 0]
    np.testing.assert_allclose(dt[:-1], 2.5e-3, rtol=1e-12)
    assert 0 < dt[-1] <= 2.5e-3 + 1e-15
    np.testing.assert_allclose(dt.sum(), 1 / 15.0, rtol=1e-12)


def test_oracle_repropagation_at_the_linearisation_point_changes_nothing(cfg, ocfg):
    """A record integrated at ba/bg/rho = the state's biases has no first-order correction to apply: the cost is the plain one."""
    w = _window(cfg, ocfg, n_landmarks=30, seed=3)
    w.speed_bias[:10, 3:9] = w.lin[:, :6]
    w.leg_bias[:10] = w.lin[:, 6:]
    plain = O.window_cost(ocfg, w)
    with O.repropagation(w):
        again = O.window_cost(ocfg, w)
    np.testing.assert_allclose(again, plain, rtol=1e-12)


def test_oracle_repropagation_replaces_the_first_order_bias_correction(cfg, ocfg):
    """Away from the linearisation point the plain factor corrects delta_p/q/v/eps to first order in the bias change; integrating
    again is exact: the two costs differ, by much less than the bias change moved the cost."""
    w = _window(cfg, ocfg, n_landmarks=30, seed=3)
    c0 = O.window_cost(ocfg, w)
    rng = np.random.default_rng(0)
    w.speed_bias[:, 3:6] += 2e-2 * rng.normal(size=(11, 3))
    w.speed_bias[:, 6:9] += 2e-3 * rng.normal(size=(11, 3))
    w.leg_bias += 2e-3 * rng.normal(size=(11, 4))
    plain = O.window_cost(ocfg, w)
    with O.repropagation(w):
        again = O.window_cost(ocfg, w)
    assert again != plain
    assert abs(again - plain) < 0.05 * abs(plain - c0)
    # and the hook is off again
    np.testing.assert_array_equal(O.window_cost(ocfg, w), plain)


def test_oracle_solve_with_repropagation_lands_next_to_the_plain_solution(cfg, ocfg):
    w1 = _window(cfg, ocfg, n_landmarks=40, seed=5)
    w2 = _window(cfg, ocfg, n_landmarks=40, seed=5)
    s1 = O.solve_window(ocfg, w1, O.default_opts(True, 6))
    with O.repropagation(w2):
        s2 = O.solve_window(ocfg, w2, O.default_opts(True, 6))
    assert s2.final_cost < s2.initial_cost
    np.testing.assert_allclose(s2.initial_cost, s1.initial_cost, rtol=1e-9)   # biases ~1e-2 from the records' linearisation point
    assert s2.initial_cost != s1.initial_cost
    np.testing.assert_allclose(s2.final_cost, s1.final_cost, rtol=1e-3)
    assert np.abs(w1.pose - w2.pose).max() < 1e-4
    assert not np.array_equal(w1.speed_bias, w2.speed_bias)


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("seed,L", [(5, 40), (6, 120)])
def test_gpu_solve_with_repropagation_vs_oracle(ctx, cfg, ocfg, seed, L):
    from cerberus_amd import api
    w_g = _window(cfg, ocfg, n_landmarks=L, seed=seed)
    w_o = _window(cfg, ocfg, n_landmarks=L, seed=seed)
    w_p = _window(cfg, ocfg, n_landmarks=L, seed=seed)
    opts = api.default_solve_opts(True, 6)
    b = api.Batch(ctx, [w_g])
    try:
        b.set_samples()
        b.solve(opts)
        sg = b.download()[0]
        # the same batch without: the records it was created with are back (re-propagation had overwritten them with the integration at
        # the last candidate point), sqrt_info and the bad-covariance flags prepared again: the plain solve, bit for bit
        b.set_samples(False)
        b.reset()
        b.solve(opts)
        s_back = b.download()[0]
        back = [a.copy() for a in w_g.state_arrays()]
        b.set_samples()   # (and on again: the integration restarts from the restored records' samples)
        b.reset()
        b.solve(opts)
        sg2 = b.download()[0]
    finally:
        b.close()
    assert sg2.final_cost == sg.final_cost
    w_b = _window(cfg, ocfg, n_landmarks=L, seed=seed)
    s_plain = ctx.solve_windows([w_b], opts)[0]
    assert s_back.final_cost == s_plain.final_cost and list(s_back.cost_trace[:7]) == list(s_plain.cost_trace[:7])
    for a, bb in zip(back, w_b.state_arrays()):
        np.testing.assert_array_equal(a, bb)

    with O.repropagation(w_o):
        so = O.solve_window(ocfg, w_o, O.default_opts(True, 6))
    assert (sg.iterations, sg.num_successful) == (so.iterations, so.num_successful)
    np.testing.assert_allclose(sg.initial_cost, so.initial_cost, rtol=1e-9)
    np.testing.assert_allclose(sg.final_cost, so.final_cost, rtol=1e-7)
    for a, bb in zip(w_g.state_arrays(), w_o.state_arrays()):
        if a.size:
            assert np.abs(a - bb).max() < 1e-8 * max(1.0, np.abs(bb).max()), np.abs(a - bb).max()
    # it is a different problem from the one with records integrated once
    sp = ctx.solve_windows([w_p], opts)[0]
    assert abs(sp.final_cost - sg.final_cost) > 1e-9 * sg.final_cost


@pytest.mark.gpu
def test_gpu_samples_off_again_restores_records_and_failed_windows(ctx, cfg, ocfg):
    """vilo_batch_set_samples(NULL) after a re-propagated solve: the records the batch was created with, their preparation and the
    per-window "a covariance has no sqrt_info" flag are back, and the launch sequence captured with the samples in force is not
    replayed: the plain solve again, bit for bit, for a window that solves and for one that fails."""
    import ctypes
    from cerberus_amd import api
    good = _window(cfg, ocfg, n_landmarks=40, seed=5)
    bad = good.twin()
    bad.preint = bad.preint.copy()
    bad.preint[2][33 + 961] = -1.0   # covariance (0, 0) of interval 2: not positive definite, no sqrt_info
    ws = [good, bad]
    opts = api.default_solve_opts(True, 4)

    def result(b):
        summ = b.download()
        return [bytes(ctypes.string_at(ctypes.addressof(s), ctypes.sizeof(s))) for s in summ], [w.clone_state() for w in ws], summ
    b = api.Batch(ctx, ws)
    try:
        b.solve(opts)
        plain_bytes, plain_states, summ = result(b)
        assert summ[1].termination == 2 and summ[0].termination != 2
        b.set_samples()
        b.reset()
        b.solve(opts)
        b.set_samples(False)
        b.reset()
        b.solve(opts)
        back_bytes, back_states, _ = result(b)
    finally:
        b.close()
    for i in range(2):
        assert back_bytes[i] == plain_bytes[i], i
        for a, bb in zip(back_states[i], plain_states[i]):
            np.testing.assert_array_equal(a, bb)


@pytest.mark.gpu
def test_gpu_repropagated_batch_of_windows_equals_the_single_solves(ctx, cfg, ocfg):
    """Interval offsets of a batch are global: every window integrates its own samples."""
    from cerberus_amd import api
    opts = api.default_solve_opts(True, 4)
    ws = [_window(cfg, ocfg, n_landmarks=40 + 10 * i, seed=20 + i) for i in range(5)]
    alone = [_window(cfg, ocfg, n_landmarks=40 + 10 * i, seed=20 + i) for i in range(5)]
    b = api.Batch(ctx, ws)
    try:
        b.set_samples()
        b.solve(opts)
        b.download()
    finally:
        b.close()
    for w in alone:
        b1 = api.Batch(ctx, [w])
        try:
            b1.set_samples()
            b1.solve(opts)
            b1.download()
        finally:
            b1.close()
    for w, w1 in zip(ws, alone):
        for a, bb in zip(w.state_arrays(), w1.state_arrays()):
            np.testing.assert_array_equal(a, bb)


@pytest.mark.gpu
def test_gpu_marginalisation_after_a_repropagated_solve_vs_oracle(ctx, cfg, ocfg):
    """The prior is linearised with the intervals integrated again at the accepted state (which the last, possibly rejected, candidate
    of the solve need not be)."""
    from cerberus_amd import api
    from cerberus_amd.synth import PriorData
    w_g = _window(cfg, ocfg, n_landmarks=50, seed=8)
    w_o = _window(cfg, ocfg, n_landmarks=50, seed=8)
    opts = api.default_solve_opts(True, 5)
    pg, po = PriorData(), PriorData()
    b = api.Batch(ctx, [w_g])
    try:
        b.set_samples()
        b.solve(opts)
        b.download()
        b.marginalize([0], [pg])
    finally:
        b.close()
    with O.repropagation(w_o):
        O.solve_window(ocfg, w_o, O.default_opts(True, 5))
        w_o.set_state(w_g.clone_state())   # the same linearisation point for the two marginalisations
        rc, m = O.marginalize(ocfg, w_o, 0, po)[:2]
    assert rc == 0 and pg.struct.valid == 1 and pg.blocks() == po.blocks()
    n = pg.n
    Jg, Jo = pg.J0_matrix(), po.J0_matrix()
    Ag, Ao = Jg.T @ Jg, Jo.T @ Jo
    assert np.abs(Ag - Ao).max() < 1e-6 * np.abs(Ao).max()
    bg, bo = Jg.T @ pg.r0[:n], Jo.T @ po.r0[:n]
    assert np.abs(bg - bo).max() < 1e-6 * np.abs(bo).max()


@pytest.mark.gpu
def test_gpu_config3_as_the_bench_times_it_vs_oracle(ctx, cfg, ocfg):
    """BASELINE configs[2] in the combination bench.py --config 3 times: 1000 landmarks (NUM_OF_F, parameters.h:24) x 400 Hz x every
    interval integrated again in every iteration (imu_leg_integration_base.cpp:62-86) x 12 fixed iterations, in a batch large enough for
    the throughput forms of every kernel (walking visual linearisation, single-wave solver: > 512 windows). First and last window of the
    batch against the oracle on the same seeds."""
    from cerberus_amd import api
    W = 520
    ws = [_window(cfg, ocfg, n_landmarks=1000, seed=700 + i) for i in range(W)]
    opts = api.default_solve_opts(True, 12)
    b = api.Batch(ctx, ws)
    try:
        b.set_samples()
        b.solve(opts)
        summ = b.download()
    finally:
        b.close()
    assert all(s.iterations == 12 for s in summ)
    for i in (0, W - 1):
        w_o = _window(cfg, ocfg, n_landmarks=1000, seed=700 + i)
        with O.repropagation(w_o):
            so = O.solve_window(ocfg, w_o, O.default_opts(True, 12))
        assert (summ[i].iterations, summ[i].num_successful) == (so.iterations, so.num_successful)
        np.testing.assert_allclose(summ[i].final_cost, so.final_cost, rtol=1e-8)
        for a, bb in zip(ws[i].state_arrays(), w_o.state_arrays()):
            if a.size:
                err = np.abs(a - bb).max() / max(1.0, np.abs(bb).max())
                print("MEASURED test_gpu_config3_as_the_bench_times_it_vs_oracle window %d: %.2e" % (i, err))
                assert err < 1e-8, (i, err)


@pytest.mark.gpu
def test_gpu_solve_with_repropagation_and_the_force_based_contact_model_vs_oracle(cfg, ocfg):
    """contact_sensor_type 2 (the go1 configurations): every re-integration is a repropagate() on an object whose contact-force filter
    carries over from pass to pass (imu_leg_integration_base.cpp:62-86 does not reset it; golden: tests/golden/preint_force_model_reprop.npz).
    Both sides integrate once per point the solver evaluates, so the passes line up: trajectories and states agree like the flag-based
    model's — and differ from a solve whose re-integrations restart the filter."""
    import copy
    from cerberus_amd import api
    from test_oracle_vs_reference import force_samples
    c2, o2 = copy.copy(cfg), copy.copy(ocfg)
    c2.contact_sensor_type = 2
    o2.contact_sensor_type = 2
    ctx2 = api.Context(c2, 0)

    def window():
        w = _window(c2, o2, n_landmarks=60, seed=9)
        w.samples[...] = force_samples(w.samples, seed=4)
        O.fill_preint(o2, w)
        return w
    w_g, w_o = window(), window()
    opts = api.default_solve_opts(True, 5)
    b = api.Batch(ctx2, [w_g])
    try:
        b.set_samples()
        b.solve(opts)
        sg = b.download()[0]
        first_states = [a.copy() for a in w_g.state_arrays()]
        # reset + solve again is the same solve, bit for bit: vilo_batch_reset brings back the contact-force filters as the objects' first
        # integration left them, not as the last solve's re-integrations did
        b.reset()
        b.solve(opts)
        sg_again = b.download()[0]
        assert sg_again.final_cost == sg.final_cost and list(sg_again.cost_trace[:6]) == list(sg.cost_trace[:6])
        for a, bb in zip(w_g.state_arrays(), first_states):
            np.testing.assert_array_equal(a, bb)
    finally:
        b.close()
        ctx2.close()
    with O.repropagation(w_o):
        so = O.solve_window(o2, w_o, O.default_opts(True, 5))
    assert (sg.iterations, sg.num_successful) == (so.iterations, so.num_successful)
    np.testing.assert_allclose(sg.initial_cost, so.initial_cost, rtol=1e-9)
    np.testing.assert_allclose(list(sg.cost_trace[:6]), list(so.cost_trace[:6]), rtol=1e-7)
    for a, bb in zip(w_g.state_arrays(), w_o.state_arrays()):
        if a.size:
            err = np.abs(a - bb).max() / max(1.0, np.abs(bb).max())
            assert err < 1e-7, err
    # a filter that restarted with every pass gives another problem: the initial cost already differs (pass 2 starts from pass 1's state)
    w_f = window()
    first = np.array([O.preintegrate_imu_leg(o2, w_f.samples[w_f.sample_offsets[k]:w_f.sample_offsets[k + 1]],
                                             np.concatenate([w_f.speed_bias[k, 3:9], w_f.leg_bias[k]])) for k in range(10)])
    w_f.preint[...] = first
    assert abs(O.window_cost(o2, w_f) - so.initial_cost) > 1e-6 * so.initial_cost
