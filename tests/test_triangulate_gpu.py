"""GPU (-m gpu): vilo_batch_triangulate / vilo_window_triangulate against the numpy definition (tests/tri_ref.py) at the state the device
returns: both branches on the packing shapes, the selections, the init_depth fallback, the back-shift, freedom from side effects, the
write-back and the solve that follows it, independence of batch size and position, the host form, the call's device memory, bad arguments.
Tolerances: ten times the FP64 floor tests/test_triangulate.py measures (tri_ref.TOL_STEREO / TOL_TWO_FRAME on |d depth| / depth,
tri_ref.TOL_SHIFT on the back-shift of given inverse depths)."""
import ctypes as C
import os

import numpy as np
import pytest

import tri_ref
from test_covariance_gpu import _window
from test_landmark_covariance_gpu import _no_landmarks
from test_triangulate import (REF, SHAPES, Z_CLEAR, fw_back_shift, mirrored, ref_globals, shape_window, third_mono)

pytestmark = pytest.mark.gpu

SEL, STE, FALL, NFIN = tri_ref.SELECTED, tri_ref.STEREO, tri_ref.FALLBACK, tri_ref.NOT_FINITE


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


def _part(r, i):
    a, b = r.offsets[i], r.offsets[i + 1]
    return [r.depth[a:b], r.flags[a:b]] + ([r.shift_inv_depth[a:b]] if r.shift_inv_depth is not None else [])


def _bitwise(x, y):
    for a, b in zip(x, y):
        assert a.shape == b.shape
        assert a.tobytes() == b.tobytes()


def _check_parity(r, i, w, tag, **kw):
    """window i of the report against the definition at w's state arrays: no landmark is left out"""
    a, b = r.offsets[i], r.offsets[i + 1]
    ref = tri_ref.window_triangulation(w, **kw)
    sel = (ref["flags"] & SEL) != 0
    assert (np.abs(ref["z"][sel]) > Z_CLEAR).all(), tag   # clear of the `depth > 0` branch, on the reference's values
    np.testing.assert_array_equal(r.flags[a:b], ref["flags"], err_msg=tag)
    es, et = tri_ref.branch_errors(r.depth[a:b], ref)
    print("MEASURED %s: stereo %.1e (tolerance %.0e), two-frame %.1e (tolerance %.0e)" % (tag, es, tri_ref.TOL_STEREO, et, tri_ref.TOL_TWO_FRAME))
    assert es <= tri_ref.TOL_STEREO and et <= tri_ref.TOL_TWO_FRAME, (tag, es, et)
    np.testing.assert_array_equal(r.depth[a:b][~sel], 1.0 / w.inv_depth[~sel])
    fall = (ref["flags"] & FALL) != 0
    np.testing.assert_array_equal(r.depth[a:b][fall], ref["depth"][fall])   # init_depth itself
    if r.shift_inv_depth is not None and not kw.get("write"):
        sh = tri_ref.back_shift(w, w.inv_depth, kw.get("init_depth", 5.0))
        e = np.abs(r.shift_inv_depth[a:b] - sh) / np.abs(sh)
        print("MEASURED %s: back-shift %.1e (tolerance %.0e)" % (tag, e.max() if e.size else 0.0, tri_ref.TOL_SHIFT))
        assert (e <= tri_ref.TOL_SHIFT).all(), (tag, e.max())
        other = w.lm_start_frame != 0
        np.testing.assert_array_equal(r.shift_inv_depth[a:b][other], w.inv_depth[other])


@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_parity_with_numpy(ctx, shape):
    from cerberus_amd import api
    ws = [shape_window(shape).twin(), third_mono(shape_window(shape))]
    b = api.Batch(ctx, ws)
    for state in ("initial", "solved"):
        if state == "solved":
            b.solve(api.default_solve_opts(True, 4))
            b.download()
        for i, name in enumerate(("stereo", "third mono")):
            _check_parity(b.triangulate("all", shift=True), i, ws[i], "%s %s %s" % (shape, name, state), select="all")
        _check_parity(b.triangulate("all", stereo=False), 0, ws[0], "%s stereo off %s" % (shape, state), select="all", stereo=False)


def test_window_without_landmarks(ctx, cfg, ocfg):
    from cerberus_amd import api
    e0 = _no_landmarks(_window(cfg, ocfg, seed=62, L=10))
    r = api.Batch(ctx, [e0.twin()]).triangulate("all", shift=True)
    assert list(r.offsets) == [0, 0] and r.depth.size == 0
    # the C entry point on such a batch: status 0 and the caller's arrays untouched
    b = api.Batch(ctx, [e0.twin(), e0.twin()])
    d, f = np.full(3, 7.0), np.full(3, 9, np.uint8)
    assert api.lib().vilo_batch_triangulate(ctx.h, b.handle, None, None, d.ctypes.data_as(C.POINTER(C.c_double)),
                                            f.ctypes.data_as(C.POINTER(C.c_uint8)), None) == 0
    assert (d == 7.0).all() and (f == 9).all()
    assert api.lib().vilo_batch_triangulate(ctx.h, b.handle, None, None, None, None, None) == 0
    # beside windows that have landmarks
    w = shape_window("L9")
    alone = api.Batch(ctx, [w.twin()]).triangulate("all", shift=True)
    mixed = api.Batch(ctx, [e0.twin(), w.twin(), e0.twin()]).triangulate("all", shift=True)
    assert list(mixed.offsets) == [0, 0, 9, 9]
    _bitwise(_part(mixed, 1), _part(alone, 0))


def test_selection(ctx, cfg, ocfg):
    from cerberus_amd import api
    ws = [shape_window("L70").twin(), shape_window("L9").twin()]
    unset = [np.array([0, 3, 17, 64, 69]), np.array([8])]
    for w, u in zip(ws, unset):
        w.inv_depth[u] = -1.0
    b = api.Batch(ctx, ws)
    r = b.triangulate()   # select = "unset"
    for i, (w, u) in enumerate(zip(ws, unset)):
        assert list(np.flatnonzero(_part(r, i)[1] & SEL)) == list(u)
        _check_parity(r, i, w, "unset %d" % i, select="unset")
    m = np.zeros(79, np.uint8)
    m[[1, 2, 40, 69, 70, 78]] = 1
    r = b.triangulate("mask", mask=m)
    np.testing.assert_array_equal((r.flags & SEL) != 0, m != 0)
    for i, w in enumerate(ws):
        _check_parity(r, i, w, "mask %d" % i, select="mask", mask=m[r.offsets[i]:r.offsets[i + 1]])
    # the negative depths of the residual report, re-initialised
    neg = (b.residuals().lm_flags & 2) != 0
    assert list(np.flatnonzero(neg)) == list(unset[0]) + [70 + 8]
    r = b.triangulate("mask", mask=neg, write=True)
    np.testing.assert_array_equal((r.flags & SEL) != 0, neg)
    before = [w.inv_depth.copy() for w in ws]
    b.download()
    after = np.concatenate([w.inv_depth for w in ws])
    np.testing.assert_array_equal(after[neg], 1.0 / r.depth[neg])
    np.testing.assert_array_equal(after[~neg], np.concatenate(before)[~neg])
    assert (after > 0).all() and not (b.residuals().lm_flags & 2).any()


@pytest.mark.parametrize("init_depth", [5.0, 2.5])
def test_fallback(ctx, init_depth):
    from cerberus_amd import api
    w, mir = mirrored(third_mono(shape_window("L70")))
    b = api.Batch(ctx, [w])
    for stereo in (True, False):
        r = b.triangulate("all", init_depth=init_depth, stereo=stereo)
        ref = tri_ref.window_triangulation(w, "all", init_depth=init_depth, stereo=stereo)
        # the mirrored points sit at localPoint.z() = -1 / inv_depth, two metres and more behind the camera
        assert (ref["z"][mir] < -1.0).all()
        assert ((r.flags[mir] & FALL) != 0).all() and (r.depth[mir] == init_depth).all() and not (r.flags & NFIN).any()
        _check_parity(r, 0, w, "fallback %g %s" % (init_depth, stereo), select="all", init_depth=init_depth, stereo=stereo)


def test_back_shift(ctx):
    from cerberus_amd import api
    w = third_mono(shape_window("L70"))
    w.inv_depth[[0, 7]] = -0.5   # frame-0 landmarks behind the camera: the back-shift's own fallback
    b = api.Batch(ctx, [w])
    r = b.triangulate("mask", mask=np.zeros(w.L, np.uint8), shift=True, init_depth=2.5)   # nothing selected: the shift of the state's depths
    _check_parity(r, 0, w, "back-shift", select="mask", mask=np.zeros(w.L, np.uint8), init_depth=2.5)
    assert (r.shift_inv_depth[[0, 7]] == 1.0 / 2.5).all()
    if os.path.exists(REF):
        lib = C.CDLL(REF)
        with ref_globals(lib, 1, 2.5):
            s = fw_back_shift(w, w.inv_depth, lib, "ref_fm_")
        e = np.abs(r.shift_inv_depth - s) / np.abs(s)
        assert np.isfinite(s).all() and (e <= tri_ref.TOL_SHIFT).all(), e.max()
    # after a write-back: the shift of the inverse depths the call leaves
    r = b.triangulate("all", write=True, shift=True)
    b.download()
    np.testing.assert_array_equal(w.inv_depth, 1.0 / r.depth)
    sh = tri_ref.back_shift(w, w.inv_depth)
    assert (np.abs(r.shift_inv_depth - sh) <= tri_ref.TOL_SHIFT * np.abs(sh)).all()
    other = w.lm_start_frame != 0
    np.testing.assert_array_equal(r.shift_inv_depth[other], w.inv_depth[other])


def _sequence(ctx, base, opts, report, samples):
    from cerberus_amd import api
    ws = [w.twin() for w in base]
    b = api.Batch(ctx, ws)
    if samples:
        b.set_samples()
    b.solve(opts)
    summ0 = b.download()
    before = [s.copy() for w in ws for s in w.state_arrays()]
    if report:
        b.triangulate("all", shift=True)
        b.triangulate()
        summ1 = b.download()
        for x, y in zip(before, [s.copy() for w in ws for s in w.state_arrays()]):
            np.testing.assert_array_equal(x, y)
        for s0, s1 in zip(summ0, summ1):
            assert bytes(s0) == bytes(s1)
    b.solve(opts)
    summ = b.download()
    return [s.copy() for w in ws for s in w.state_arrays()], [bytes(s) for s in summ]


@pytest.mark.parametrize("samples", [False, True])
def test_no_side_effects(ctx, cfg, ocfg, samples):
    from cerberus_amd import api
    base = [_window(cfg, ocfg, seed=s) for s in (11, 12)]
    opts = api.default_solve_opts(True, 4)
    st_a, su_a = _sequence(ctx, base, opts, False, samples)
    st_b, su_b = _sequence(ctx, base, opts, True, samples)
    for x, y in zip(st_a, st_b):
        np.testing.assert_array_equal(x, y)
    assert su_a == su_b


@pytest.mark.parametrize("solved_before", [False, True])
def test_write_back(ctx, solved_before):
    from cerberus_amd import api
    opts = api.default_solve_opts(True, 4)
    base = [third_mono(shape_window("L70")), shape_window("L9").twin()]
    ws = [w.twin() for w in base]
    sel = np.zeros(79, np.uint8)
    sel[::2] = 1
    b = api.Batch(ctx, ws)
    if solved_before:
        b.solve(opts)
        b.reset()
    b.download()
    before = [[a.copy() for a in w.state_arrays()] for w in ws]
    r = b.triangulate("mask", mask=sel, write=True)
    b.download()
    for i, w in enumerate(ws):
        m = sel[r.offsets[i]:r.offsets[i + 1]] != 0
        for x, y in zip(before[i][:5], w.state_arrays()[:5]):
            np.testing.assert_array_equal(x, y)   # the camera-side state
        np.testing.assert_array_equal(w.inv_depth[m], 1.0 / _part(r, i)[0][m])
        np.testing.assert_array_equal(w.inv_depth[~m], before[i][5][~m])
        assert (w.inv_depth[m] != before[i][5][m]).any()
    # the solve that follows starts from the new values: a fresh batch with them as initial state gives the same, bit for bit
    fresh = [w.twin() for w in ws]
    b.solve(opts)
    assert b.path()["replay"] == solved_before
    summ = b.download()
    fb = api.Batch(ctx, fresh)
    fb.solve(opts)
    assert not fb.path()["replay"]
    fsumm = fb.download()
    for w, f in zip(ws, fresh):
        for x, y in zip(w.state_arrays(), f.state_arrays()):
            np.testing.assert_array_equal(x, y)
    assert [bytes(s) for s in summ] == [bytes(s) for s in fsumm]
    # the uploaded initial state is still what reset restores
    b.reset()
    b.download()
    for w, o in zip(ws, base):
        for x, y in zip(w.state_arrays(), o.state_arrays()):
            np.testing.assert_array_equal(x, y)


def test_independent_of_batch_size_and_position(ctx, cfg, ocfg):
    from cerberus_amd import api
    w = third_mono(shape_window("L70"))
    other = _window(cfg, ocfg, seed=78, L=200)
    alone = _part(api.Batch(ctx, [w.twin()]).triangulate("all", shift=True), 0)
    eight = [other.twin() for _ in range(8)]
    eight[3] = w.twin()
    _bitwise(_part(api.Batch(ctx, eight).triangulate("all", shift=True), 3), alone)
    many = [other.twin() for _ in range(300)]
    for pos in (0, 150, 299):
        many[pos] = w.twin()
    r = api.Batch(ctx, many).triangulate("all", shift=True)
    for pos in (0, 150, 299):
        _bitwise(_part(r, pos), alone)


def test_host_window_form_matches_batch(ctx):
    from cerberus_amd import api
    ws = [third_mono(shape_window("L70")), shape_window("L9").twin(), shape_window("F6").twin()]
    for w in ws:
        w.inv_depth[::5] = -1.0
    r = api.Batch(ctx, [w.twin() for w in ws]).triangulate(shift=True)
    h = ctx.window_triangulate(ws, shift=True)
    for i in range(3):
        _bitwise(_part(h, i), _part(r, i))
    np.testing.assert_array_equal(np.concatenate([w.inv_depth for w in ws])[::5][:2], -1.0)   # write = 0: the windows are left alone
    b = api.Batch(ctx, [w.twin() for w in ws])
    r = b.triangulate(shift=True, write=True)
    tw = [w.twin() for w in ws]
    h = ctx.window_triangulate(tw, shift=True, write=True)
    for i in range(3):
        _bitwise(_part(h, i), _part(r, i))
        sel = (_part(r, i)[1] & SEL) != 0
        np.testing.assert_array_equal(tw[i].inv_depth[sel], 1.0 / _part(r, i)[0][sel])
        np.testing.assert_array_equal(tw[i].inv_depth[~sel], ws[i].inv_depth[~sel])
        for x, y in zip(tw[i].state_arrays()[:5], ws[i].state_arrays()[:5]):
            np.testing.assert_array_equal(x, y)


def test_device_memory_is_returned(ctx, cfg, ocfg):
    from cerberus_amd import api
    b = api.Batch(ctx, [_window(cfg, ocfg, seed=s, L=50) for s in (13, 14)])
    bytes0 = b.device_bytes()   # nothing is kept with the batch: not even at the first call
    first = b.triangulate("all", shift=True)
    assert b.device_bytes() == bytes0
    m = np.ones(100, np.uint8)
    for _ in range(5):
        r = b.triangulate("mask", mask=m, shift=True)
        assert b.device_bytes() == bytes0
    for i in range(2):
        _bitwise(_part(r, i), _part(first, i))


def test_bad_arguments(ctx):
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    w = shape_window("L9").twin()
    b = api.Batch(ctx, [w])
    f = api.lib().vilo_batch_triangulate
    d, fl, m = np.zeros(9), np.zeros(9, np.uint8), np.ones(9, np.uint8)
    dp_, fp, mp = d.ctypes.data_as(T.c_double_p), T.u8ptr(fl), T.u8ptr(m)

    def opts(**kw):
        o = T.TriangulateOpts()
        api.lib().vilo_default_triangulate_opts(C.byref(o))
        for k, v in kw.items():
            setattr(o, k, v)
        return C.byref(o)
    o = T.TriangulateOpts()
    api.lib().vilo_default_triangulate_opts(C.byref(o))
    assert (o.init_depth, o.stereo, o.select, o.write, o.pad) == (5.0, 1, 0, 0, 0)
    assert f(None, b.handle, opts(), None, dp_, fp, None) == -2
    assert f(ctx.h, None, opts(), None, dp_, fp, None) == -2
    assert f(ctx.h, b.handle, opts(select=2), None, dp_, fp, None) == -2          # MASK without a mask
    assert f(ctx.h, b.handle, opts(select=1), None, None, fp, None) == -2         # NULL depth with landmarks present
    for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
        assert f(ctx.h, b.handle, opts(init_depth=bad), None, dp_, fp, None) == -2
    for bad in (3, -1):
        assert f(ctx.h, b.handle, opts(select=bad), mp, dp_, fp, None) == -2
    g = api.lib().vilo_window_triangulate
    ds, ss = w.desc(T)
    assert g(ctx.h, 0, C.byref(ds), C.byref(ss), opts(), None, dp_, fp, None) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(select=2), None, dp_, fp, None) == -2
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(init_depth=-2.0), None, dp_, fp, None) == -2
    assert not d.any() and not fl.any()
    # the batch is still usable; NULL options are the defaults, flags and the shift may be left out
    assert f(ctx.h, b.handle, None, None, dp_, None, None) == 0
    np.testing.assert_array_equal(d, 1.0 / w.inv_depth)
    assert f(ctx.h, b.handle, opts(select=2), mp, dp_, fp, None) == 0 and (fl & SEL).all()
    assert api.lib().vilo_last_triangulate_ms(ctx.h) > 0.0
    assert g(ctx.h, 1, C.byref(ds), C.byref(ss), opts(select=1), None, dp_, fp, None) == 0
    _check_parity(b.triangulate("all"), 0, w, "after bad arguments", select="all")
