"""GPU (-m gpu): vilo_batch_repropagate / vilo_window_repropagate. The re-propagated records against vilo_preintegrate bit for bit and
against the oracle's repropagate at tests/test_gpu_parity.py::test_preintegrate's bounds (contact models 0 and 1, the alternative
configuration); the solve that follows against the solve of a fresh batch built from those records, bit for bit, plain launches and graph
replay; drifts, `selected` and statuses against the numpy definition (tests/reprop_ref.py; drifts within reprop_ref.TOL); what a
selection leaves alone; the start-up sequence against the oracle's ratio; independence of batch size and position; the call's device
memory; NUMERIC, NO_SAMPLES, VILO_ERR_UNSUPPORTED, bad arguments; a compact-uploaded batch; the host form.
A batch whose records were gathered from a vilo_preint_streams pool exists only inside vilo_optimize_windows_resident (no public call
creates one), so that VILO_ERR_UNSUPPORTED cannot be reached from here."""
import ctypes as C

import numpy as np
import pytest

import reprop_ref as R

pytestmark = pytest.mark.gpu

LEG_D, IMU_D, PREP_D = 33 + 2 * 961, 17 + 2 * 225, 126 + 961


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _records(b, i, w):
    return b.fetch(13, i).reshape(10, LEG_D) if w.use_leg else b.fetch(16, i).reshape(10, IMU_D)


def _prepared(b, i):
    return b.fetch(15, i).reshape(10, PREP_D)


def _expected(ctx, w, rows):
    """vilo_preintegrate / vilo_preintegrate_imu of the window's samples at rows [10, 10]: [F - 1] records"""
    n = w.F - 1
    smp, off = w.samples[:int(w.sample_offsets[n])], w.sample_offsets[:n + 1]
    if w.use_leg:
        return ctx.preintegrate(smp, off, np.ascontiguousarray(rows[:n]))
    return ctx.preintegrate_imu(smp, off, np.ascontiguousarray(rows[:n, :6]))


def _rows(w, point, lin=None):
    return R.evaluate(w, R.record_lin(w), point=point, lin=lin).rows


def _state(ws):
    return [a.tobytes() for w in ws for a in w.state_arrays()]


def _with_records(w, rec):
    t = w.twin()
    if w.use_leg:
        t.preint = w.preint.copy()
        t.preint[:w.F - 1] = rec
    else:
        t.preint_imu = w.preint_imu.copy()
        t.preint_imu[:w.F - 1] = rec
    return t


@pytest.mark.parametrize("point", R.POINTS)
@pytest.mark.parametrize("group", ["leg", "imu"])
def test_records_are_vilo_preintegrate_bit_for_bit(ctx, group, point):
    from cerberus_amd import api
    ws = [R.case_window(n).twin() for n in (R.LEG_CASES if group == "leg" else R.IMU_CASES)]
    lin = np.stack([R.given_rows(w) for w in ws]) if point == "given" else None
    b = api.Batch(ctx, ws)
    before = [_records(b, i, w).copy() for i, w in enumerate(ws)]
    r = b.repropagate(point=point, lin=lin)
    assert api.lib().vilo_last_repropagate_ms(ctx.h) > 0.0
    for i, w in enumerate(ws):
        n = w.F - 1
        assert list(r.status[i]) == [R.OK] * n + [R.NO_INTERVAL] * (10 - n) and list(r.selected[i]) == [1] * n + [0] * (10 - n)
        rows = _rows(w, point, None if lin is None else lin[i])
        got, want = _records(b, i, w), _expected(ctx, w, rows)
        assert got[:n].tobytes() == want.tobytes(), (group, point, i)
        assert got[:n].tobytes() != before[i][:n].tobytes()
        assert got[n:].tobytes() == before[i][n:].tobytes()
        o = 23 if w.use_leg else 11
        np.testing.assert_array_equal(got[:n, o:o + (10 if w.use_leg else 6)], rows[:n, :10 if w.use_leg else 6])
        # a second call at the same point: zero drift, the same bits
    r2 = b.repropagate(point=point, lin=lin)
    assert not r2.drift.any()
    for i, w in enumerate(ws):
        assert _records(b, i, w)[:w.F - 1].tobytes() == _expected(ctx, w, _rows(w, point, None if lin is None else lin[i])).tobytes()


@pytest.mark.parametrize("replay", [False, True])
@pytest.mark.parametrize("group", ["leg", "imu"])
def test_following_solve_is_the_fresh_batchs(ctx, group, replay):
    from cerberus_amd import api
    opts = api.default_solve_opts(True, 4)
    ws = [R.case_window(n).twin() for n in (("F11", "F6") if group == "leg" else R.IMU_CASES)]
    b = api.Batch(ctx, ws)
    if replay:
        b.solve(opts)
        b.reset()
    b.repropagate(point="startup")
    fresh = [_with_records(w, _expected(ctx, w, _rows(w, "startup"))) for w in ws]
    b.solve(opts)
    assert b.path()["replay"] == replay
    s1 = [bytes(s) for s in b.download()]
    fb = api.Batch(ctx, fresh)
    fb.solve(opts)
    s2 = [bytes(s) for s in fb.download()]
    assert _state(ws) == _state(fresh) and s1 == s2
    # reset restores the states only: the records stay
    rec = [_records(b, i, w).tobytes() for i, w in enumerate(ws)]
    b.reset()
    b.download()
    assert _state(ws) == _state([R.case_window(n) for n in (("F11", "F6") if group == "leg" else R.IMU_CASES)])
    assert rec == [_records(b, i, w).tobytes() for i, w in enumerate(ws)]


def _rel(a, b):
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.mark.parametrize("config", ["type0", "type1", "alt"])
def test_against_the_oracles_repropagate(cfg, config):
    """the bounds of tests/test_gpu_parity.py::test_preintegrate, at the start-up point"""
    import alt_config
    from cerberus_amd import api
    from oracle import oracle_py as O
    c = {"type0": alt_config.with_type(cfg, 0), "type1": alt_config.with_type(cfg, 1), "alt": alt_config.alt_config(cfg)}[config]
    oc = O.config_from(c)
    cx = api.Context(c, 0)
    try:
        for name in ("F11", "F6"):
            w = R.case_window(name).twin()
            b = api.Batch(cx, [w])
            assert (b.repropagate(point="startup").status[0, :w.F - 1] == R.OK).all()
            got, rows = _records(b, 0, w), _rows(w, "startup")
            ej = ec = 0.0
            for k in range(w.F - 1):
                a0, a1 = w.sample_offsets[k], w.sample_offsets[k + 1]
                a, o = got[k], O.repropagate_imu_leg(oc, w.samples[a0:a1], w.lin[k], [rows[k]])[1]
                np.testing.assert_allclose(a[:33], o[:33], rtol=1e-12, atol=1e-14, err_msg="state k=%d" % k)
                assert _rel(a[33:33 + 961], o[33:33 + 961]) < 1e-11, ("jacobian", k)
                assert _rel(a[33 + 961:], o[33 + 961:]) < 1e-10, ("covariance", k)
                ca, cb = a[33 + 961:], o[33 + 961:]
                big = np.abs(cb) > 1e-6 * np.abs(cb).max()
                assert np.abs(ca[big] / cb[big] - 1).max() < 1e-9
                ej, ec = max(ej, _rel(a[33:33 + 961], o[33:33 + 961])), max(ec, _rel(ca, cb))
                # (0, Bg_{k+1}, rho_{k+1}), not the start frame's: those records are far outside the bounds
                bad = O.preintegrate_imu_leg(oc, w.samples[a0:a1], np.concatenate([np.zeros(3), w.speed_bias[k, 6:9], w.leg_bias[k]]))
                assert (np.abs(a[:33] - bad[:33]) / (1e-12 * np.abs(bad[:33]) + 1e-14)).max() >= 1000.0
            print("MEASURED %s %s: jacobian %.1e (1e-11) covariance %.1e (1e-10)" % (config, name, ej, ec))
            b.close()
    finally:
        cx.close()


@pytest.mark.parametrize("name", R.LEG_CASES + R.IMU_CASES)
def test_drifts_selection_and_statuses_match_numpy(ctx, name):
    from cerberus_amd import api
    w = R.case_window(name).twin()
    b = api.Batch(ctx, [w])
    rec0, prep0 = _records(b, 0, w).tobytes(), _prepared(b, 0).tobytes()
    worst = 0.0
    for tag, cw, kw in R.cases():
        if not tag.startswith(name + " "):
            continue
        rl = R.record_lin(w)
        for write in (False, True):
            ref = R.evaluate(w, rl, write=write, counts=R.counts(w), **kw)
            if write:
                bb = api.Batch(ctx, [w.twin()])
                r = bb.repropagate(write=True, **kw)
            else:
                r = b.repropagate(write=False, **kw)
            scale = max(1.0, np.abs(ref.rows).max(), np.abs(rl).max())
            e = float(np.abs(r.drift[0] - ref.drift).max()) / scale
            worst = max(worst, e)
            assert e <= R.TOL, (tag, write, e)
            assert (r.selected[0] == ref.selected).all() and (r.status[0] == ref.status).all(), (tag, write, r.status[0], ref.status)
    print("MEASURED %s: largest drift error %.1e (tolerance %.0e)" % (name, worst, R.TOL))
    assert _records(b, 0, w).tobytes() == rec0 and _prepared(b, 0).tobytes() == prep0   # the drift queries wrote nothing


@pytest.mark.parametrize("select", ["drifted", "mask"])
@pytest.mark.parametrize("group", ["leg", "imu"])
def test_unselected_records_are_untouched(ctx, group, select):
    from cerberus_amd import api
    ws = [R.case_window(n).twin() for n in (("F11", "F6") if group == "leg" else R.IMU_CASES)]
    b = api.Batch(ctx, ws)
    rec0 = [_records(b, i, w).copy() for i, w in enumerate(ws)]
    prep0 = [_prepared(b, i).copy() for i in range(len(ws))]
    mask = np.stack([R.mask_of(w) for w in ws]) if select == "mask" else None
    r = b.repropagate(select=select, mask=mask, thresholds=R.THRESHOLDS)
    n_sel = n_not = 0
    for i, w in enumerate(ws):
        ref = R.evaluate(w, R.record_lin(w), select=select, mask=None if mask is None else mask[i], thresholds=R.THRESHOLDS, counts=R.counts(w))
        assert (r.selected[i] == ref.selected).all() and (r.status[i] == ref.status).all()
        got, prep, want = _records(b, i, w), _prepared(b, i), _expected(ctx, w, _rows(w, "state"))
        for k in range(10):
            if r.status[i, k] == R.OK:
                n_sel += 1
                assert got[k].tobytes() == want[k].tobytes() and got[k].tobytes() != rec0[i][k].tobytes()
                assert prep[k].tobytes() != prep0[i][k].tobytes()
            else:
                n_not += k < w.F - 1
                assert got[k].tobytes() == rec0[i][k].tobytes() and prep[k].tobytes() == prep0[i][k].tobytes(), (i, k)
    assert n_sel > 0 and n_not > 0
    # the prepared form of the whole batch is the one a fresh batch of the same records prepares
    fb = api.Batch(ctx, [_with_records(w, _records(b, i, w)[:w.F - 1]) for i, w in enumerate(ws)])
    for i, w in enumerate(ws):
        assert _prepared(fb, i)[:w.F - 1].tobytes() == _prepared(b, i)[:w.F - 1].tobytes()


def test_drift_query_leaves_the_batch_alone(ctx):
    from cerberus_amd import api
    opts = api.default_solve_opts(True, 4)
    out = []
    for query in (False, True):
        ws = [R.case_window(n).twin() for n in ("F11", "F6")]
        b = api.Batch(ctx, ws)
        if query:
            r = b.repropagate(write=False, point="startup")
            assert r.drift.any() and (r.status[0] == R.OK).all()
        b.solve(opts)
        summ = [bytes(s) for s in b.download()]
        out.append((_state(ws), summ, [_records(b, i, w).tobytes() for i, w in enumerate(ws)]))
    assert out[0] == out[1]


def test_startup_sequence(ctx):
    """gyro_bias_align(write) -> repropagate(startup) -> gyro_bias_align: |second| / |first| within ten times the oracle's ratio for the
    same sequence (reprop_ref.STARTUP_RATIO, tests/test_repropagate.py); the margin covers nothing but rounding"""
    from cerberus_amd import api
    w = R.case_window("F11").twin()
    w.speed_bias[:, 6:9] += np.array(R.STARTUP_OFFSET)
    b = api.Batch(ctx, [w])
    d1 = b.gyro_bias_align(write=True)
    r = b.repropagate(point="startup")
    d2 = b.gyro_bias_align(linearization="record")
    assert d1.status[0] == 0 and d2.status[0] == 0 and (r.status[0] == R.OK).all()
    ratio = float(np.linalg.norm(d2.delta_bg[0]) / np.linalg.norm(d1.delta_bg[0]))
    print("MEASURED start-up sequence: |d1| %.3e |d2| %.3e ratio %.6e (oracle %.6e, gate %.6e)"
          % (np.linalg.norm(d1.delta_bg[0]), np.linalg.norm(d2.delta_bg[0]), ratio, R.STARTUP_RATIO, 10 * R.STARTUP_RATIO))
    assert ratio <= 10 * R.STARTUP_RATIO


def _one(r, b, i, w):
    return (r.drift[i].tobytes(), r.selected[i].tobytes(), r.status[i].tobytes(), _records(b, i, w).tobytes(), _prepared(b, i)[:w.F - 1].tobytes())


def test_independent_of_batch_size_and_position(ctx):
    from cerberus_amd import api
    bases = [R.case_window(n) for n in R.LEG_CASES]
    alone = []
    for w in bases:
        b = api.Batch(ctx, [w.twin()])
        alone.append(_one(b.repropagate(point="startup"), b, 0, w))
    assert len({a[3] for a in alone}) == 3
    for n, look in ((8, (3,)), (300, (0, 150, 299))):
        ws = [bases[i % 3].twin() for i in range(n)]
        b = api.Batch(ctx, ws)
        r = b.repropagate(point="startup")
        for i in look:
            assert _one(r, b, i, ws[i]) == alone[i % 3], (n, i)


def test_device_memory_numeric_no_samples(ctx):
    from cerberus_amd import api
    good = R.case_window("F11")
    bad = good.twin()
    bad.speed_bias[4, 7] = np.nan
    ws = [good.twin(), bad, good.twin()]
    b = api.Batch(ctx, ws)
    bytes0 = b.device_bytes()
    rec0 = _records(b, 1, bad).copy()
    samples, offsets = api.window_samples(ws)
    offsets = offsets.copy()
    cut = offsets[22] - offsets[21] - 1     # interval 1 of window 2 keeps one sample: its range ends early, the next begins where it did
    smp = np.concatenate([samples[:offsets[21] + 1], samples[offsets[22]:]])
    offsets[22:] -= cut
    for _ in range(10):
        r = b.repropagate(smp, offsets)
        assert b.device_bytes() == bytes0
    want = [R.OK] * 10
    assert list(r.status[0]) == want
    assert list(r.status[1]) == [R.OK] * 4 + [R.NUMERIC] + [R.OK] * 5 and r.selected[1, 4] == 0 and not r.drift[1, 4].any()
    assert list(r.status[2]) == [R.OK, R.NO_SAMPLES] + [R.OK] * 8 and r.selected[2, 1] == 1
    exp = _expected(ctx, good, _rows(good, "state"))
    assert _records(b, 0, good).tobytes() == exp.tobytes()
    got = _records(b, 1, bad)
    assert got[4].tobytes() == rec0[4].tobytes()
    for k in (0, 1, 2, 3, 5, 6, 7, 8, 9):
        assert got[k].tobytes() == exp[k].tobytes()
    got2 = _records(b, 2, good)
    assert got2[1].tobytes() == rec0[1].tobytes() and got2[[0] + list(range(2, 10))].tobytes() == exp[[0] + list(range(2, 10))].tobytes()


def test_unsupported_bad_arguments_and_compact_upload(ctx):
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    w = R.case_window("F11").twin()
    b = api.Batch(ctx, [w])
    # the records went up in the compact form: the Jacobian entries no factor reads are zero, the lower triangle mirrors the upper
    assert list(b.fetch(17)) == [1.0, 0.0]
    rec = _records(b, 0, w)
    assert not rec[0, 33:33 + 21].any() and w.preint[0, 33:33 + 21].any()
    mask = np.zeros(10, np.uint8)
    mask[2] = 1
    b.repropagate(select="mask", mask=mask)
    assert list(b.fetch(17)) == [2.0, 0.0]
    b.repropagate()
    assert list(b.fetch(17)) == [0.0, 0.0]
    full = _expected(ctx, w, _rows(w, "state"))
    assert _records(b, 0, w).tobytes() == full.tobytes() and full[0, 33:33 + 21].any()
    # samples in force: the solve integrates anyway
    b.set_samples()
    with pytest.raises(api.ViloError, match="vilo_batch_set_samples is in force"):
        b.repropagate()
    b.set_samples(False)
    b.repropagate()
    f = api.lib().vilo_batch_repropagate
    samples, offsets = api.window_samples([w])
    sp, op = C.cast(samples.ctypes.data, C.POINTER(T.Sample)), T.iptr(offsets)
    rec = (T.IntervalRepropRecord * 10)()
    lin, m8 = np.zeros((10, 10)), np.ones(10, np.uint8)

    def opts(**kw):
        o = T.RepropOpts()
        api.lib().vilo_default_reprop_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    assert f(None, b.handle, sp, op, opts(), None, None, rec) == -2 and f(ctx.h, None, sp, op, opts(), None, None, rec) == -2
    for kw in (dict(point=3), dict(point=-1), dict(select=3), dict(select=-1), dict(write=2), dict(write=-1), dict(point=2), dict(select=2),
               dict(ba_threshold=-1.0), dict(bg_threshold=float("nan")), dict(rho_threshold=float("inf"))):
        assert f(ctx.h, b.handle, sp, op, opts(**kw), None, None, rec) == -2, kw
    assert f(ctx.h, b.handle, None, op, opts(), None, None, rec) == -2 and f(ctx.h, b.handle, sp, None, opts(), None, None, rec) == -2
    down = offsets.copy()
    down[5] = down[4] - 1
    neg = offsets.copy()
    neg[0] = -1
    assert f(ctx.h, b.handle, sp, T.iptr(down), opts(), None, None, rec) == -2 and f(ctx.h, b.handle, sp, T.iptr(neg), opts(), None, None, rec) == -2
    assert _records(b, 0, w).tobytes() == full.tobytes()   # (nothing of that was launched)
    # NULL options are the defaults, the records may be left out, the drift query needs no samples
    assert f(ctx.h, b.handle, sp, op, None, None, None, None) == 0
    assert f(ctx.h, b.handle, None, None, opts(write=0, point=2, select=2), T.dptr(lin), T.u8ptr(m8), rec) == 0 and rec[0].status == R.OK


def test_host_window_form(ctx):
    from cerberus_amd import api
    for names in (("F11", "F6"), R.IMU_CASES):
        ws = [R.case_window(n).twin() for n in names]
        for w in ws:
            w.preint, w.preint_imu = w.preint.copy(), w.preint_imu.copy()
        keep = [(w.preint.copy(), w.preint_imu.copy()) for w in ws]
        mask = np.stack([R.mask_of(w) for w in ws])
        q = ctx.window_repropagate(ws, write=False, point="startup")
        assert all((w.preint == k[0]).all() and (w.preint_imu == k[1]).all() for w, k in zip(ws, keep)) and q.drift.any()
        r = ctx.window_repropagate(ws, select="mask", mask=mask)
        for i, w in enumerate(ws):
            want = _expected(ctx, w, _rows(w, "state"))
            mine, other = (w.preint, w.preint_imu) if w.use_leg else (w.preint_imu, w.preint)
            assert other.tobytes() == keep[i][0 if not w.use_leg else 1].tobytes()
            for k in range(10):
                exp = want[k] if r.status[i, k] == R.OK else keep[i][0 if w.use_leg else 1][k]
                assert mine[k].tobytes() == exp.tobytes(), (names, i, k)
