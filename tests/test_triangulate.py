"""CPU: the numpy definition of vilo_batch_triangulate (tests/tri_ref.py) against the compiled reference's FeatureManager (triangulate and
removeBackShiftDepth through oracle/_ref/libref.so's ref_fm_* entry points, where that library exists) and the host library's
vilo_fw_triangulate; the measured FP64 floor that sets the GPU tolerances (tri_ref.TOL_* = 10 x tri_ref.FLOOR_*); the option
parsing of the Python wrapper. tests/test_triangulate_gpu.py takes its windows and references from here."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

import tri_ref
from conftest import ROOT
from test_covariance_gpu import _window
from test_feature_window import FW, HOST, REF, dp

SEL, STE, FALL = tri_ref.SELECTED, tri_ref.STEREO, tri_ref.FALLBACK
# localPoint.z() of every parity landmark is at least this far from the `depth > 0` branch (metres): a thousand times the widest tolerance
Z_CLEAR = 1000 * max(tri_ref.TOL_STEREO, tri_ref.TOL_TWO_FRAME)

# the packing shapes (tests/test_triangulate_gpu.py): one segment with padded lanes; several start frames packed into one wave with n not a
# multiple of 8; 66 landmarks sharing each start frame (two chunks); six frames
SHAPES = {"L9": dict(L=9, seed=501), "L70": dict(L=70, seed=502), "L456": dict(L=456, seed=503),
          "F6": dict(L=40, seed=504, F=6, prior=False, leg_bias_const=1)}


def third_mono(w):
    """the same window with obs_is_stereo cleared on the first observation of every third landmark (its own copies of the arrays)"""
    t = w.twin()
    t.obs_is_stereo = w.obs_is_stereo.copy()
    t.obs_is_stereo[w.lm_obs_offset[:-1][::3]] = 0
    return t


def mirrored(w, every=4):
    """the same window with every `every`-th landmark's point (at its inverse depth, the window's poses) mirrored through the centre of
    the start frame's left camera: the first observation's right-camera point and the second observation's left-camera point are the
    projections of the mirrored point, so both branches triangulate it exactly, at localPoint.z() = -1 / inv_depth"""
    t = w.twin()
    t.obs = w.obs.copy()
    Ps, Rs, tic, ric = tri_ref.poses(w)
    idx = np.arange(w.L)[::every]
    for l in idx:
        o, s = w.lm_obs_offset[l], int(w.lm_start_frame[l])
        Xw = Rs[s] @ (ric[0] @ (-w.obs[o, 0:3] / w.inv_depth[l]) + tic[0]) + Ps[s]
        for row, col, k, cam in ((o, 3, s, 1), (o + 1, 0, s + 1, 0)):
            p = tri_ref.projection(Ps, Rs, tic, ric, k, cam) @ np.append(Xw, 1.0)
            t.obs[row, col:col + 2] = p[:2] / p[2]
    return t, idx


@functools.lru_cache(maxsize=None)
def shape_window(name):
    from cerberus_amd import synth
    from oracle import oracle_py as O
    cfg = synth.default_config()
    return _window(cfg, O.config_from(cfg), **SHAPES[name])


@functools.lru_cache(maxsize=None)
def solved_window(name):
    """the shape's window after a 4-iteration solve by the oracle: the CPU stand-in for the state the GPU parity test reaches (the two
    agree to 1e-8; what matters here is the conditioning of the triangulation at the solved poses)"""
    from cerberus_amd import synth
    from oracle import oracle_py as O
    w = shape_window(name).twin()
    O.solve_window(O.config_from(synth.default_config()), w, O.default_opts(True, 4))
    return w


def parity_cases():
    """(tag, window, stereo option) of every parity case, at the initial state and after a 4-iteration solve: the generator's stereo
    landmarks, every third landmark two-frame, all two-frame"""
    out = []
    for name in SHAPES:
        for state, w in (("initial", shape_window(name)), ("solved", solved_window(name))):
            out += [("%s stereo %s" % (name, state), w, True), ("%s third mono %s" % (name, state), third_mono(w), True),
                    ("%s stereo off %s" % (name, state), w, False)]
    return out


# ---- the same window through a feature window of the C entry points (the reference's FeatureManager or the host library's) ----
def _fw_load(w, lib, prefix):
    fw = FW(lib, prefix)
    for fc in range(w.F):
        ids = [l for l in range(w.L) if w.lm_start_frame[l] <= fc < w.lm_start_frame[l] + w.lm_obs_offset[l + 1] - w.lm_obs_offset[l]]
        rows = [w.lm_obs_offset[l] + fc - w.lm_start_frame[l] for l in ids]
        fw.add_frame(fc, np.array(ids, np.int32), w.obs[rows], w.obs_is_stereo[rows], float(w.td[0]))
    return fw


def _fw_depths(fw, L):
    info, depth, _, _ = fw.dump()
    out = np.full(L, np.nan)
    out[info[:, 0]] = depth
    return out


def fw_triangulate(w, lib, prefix):
    """depth per landmark (the window's order) of the feature window's triangulate at the window's poses, every track unset before it"""
    fw = _fw_load(w, lib, prefix)
    fw.call("triangulate", *[np.ascontiguousarray(x).ctypes.data_as(dp) for x in tri_ref.poses(w)])
    d = _fw_depths(fw, w.L)
    fw.call("destroy")
    return d


def fw_back_shift(w, inv_depth, lib, prefix):
    """1 / depth per landmark after set_depth(inv_depth) and removeBackShiftDepth with frame 0's and frame 1's left camera; NaN for the
    tracks set_depth does not reach (fewer than four observations)"""
    fw = _fw_load(w, lib, prefix)
    n_obs = np.diff(w.lm_obs_offset)
    order = [l for l in sorted(range(w.L), key=lambda l: (w.lm_start_frame[l], l)) if n_obs[l] >= 4]   # the list order of the tracks
    assert fw.call("feature_count") == len(order)
    x = np.ascontiguousarray(inv_depth[order])
    fw.call("set_depth", x.ctypes.data_as(dp))
    Ps, Rs, tic, ric = tri_ref.poses(w)
    m = [np.ascontiguousarray(v).ctypes.data_as(dp) for v in (Rs[0] @ ric[0], Ps[0] + Rs[0] @ tic[0], Rs[1] @ ric[0], Ps[1] + Rs[1] @ tic[0])]
    fw.call("remove_back_shift_depth", *m)
    out = 1.0 / _fw_depths(fw, w.L)
    out[n_obs < 4] = np.nan
    fw.call("destroy")
    return out


class ref_globals:
    """the reference's STEREO / INIT_DEPTH globals (oracle/ref_build/ref_driver_fm.cpp) set for a block"""

    def __init__(self, lib, stereo=1, init_depth=5.0):
        self.s, self.d = C.c_int.in_dll(lib, "STEREO"), C.c_double.in_dll(lib, "INIT_DEPTH")
        self.new = (int(stereo), float(init_depth))

    def __enter__(self):
        self.old = (self.s.value, self.d.value)
        self.s.value, self.d.value = self.new

    def __exit__(self, *a):
        self.s.value, self.d.value = self.old


def _ulp_moved(w, rng):
    """the window with every pose / extrinsic entry and every observation coordinate moved by one unit in the last place, up or down"""
    t = w.twin()
    t.obs = w.obs.copy()
    for a in (t.pose, t.ex_pose, t.obs):
        a[...] = np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
    return t


def _rel(a, b, m):
    return float((np.abs(a - b)[m] / np.abs(b)[m]).max()) if m.any() else 0.0


def test_fp64_floor_measured():
    """Prints the floor of the definition per branch, |d depth| / depth over the parity windows: (a) one unit in the last place on the
    inputs, (b) the compiled reference's FeatureManager, (c) the host library's vilo_fw_triangulate; tri_ref.FLOOR_* must cover the largest.
    Measured (x86-64, numpy's LAPACK) on the initial states: stereo (a) 7.8e-13 (b) 3.4e-13 (c) 3.4e-13; two-frame (a) 8.9e-13 (b) 5.6e-13
    (c) 5.6e-13. With the states after a 4-iteration solve (the oracle's), where the 456-landmark window has landmarks that triangulate to
    1.2 km (stereo) and 1.6 km (two-frame): stereo (a) 8.8e-12 (b) 3.3e-12 (c) 3.3e-12; two-frame (a) 2.2e-11 (b) 1.5e-11 (c) 1.5e-11. The
    back-shift of a given inverse depth, the larger of (a) and (b): 8.8e-16."""
    rng = np.random.default_rng(7)
    ref_lib = C.CDLL(REF) if os.path.exists(REF) else None
    host_lib = C.CDLL(HOST)
    worst = {"a": [0.0, 0.0], "b": [0.0, 0.0], "c": [0.0, 0.0]}
    shift = 0.0
    for tag, w, stereo in parity_cases():
        r = tri_ref.window_triangulation(w, "all", stereo=stereo)
        assert (np.abs(r["z"]) > Z_CLEAR).all() and (r["flags"] & SEL).all(), tag
        st = (r["flags"] & STE) != 0
        s0 = tri_ref.back_shift(w, w.inv_depth)
        for _ in range(3):
            wm = _ulp_moved(w, rng)
            shift = max(shift, _rel(tri_ref.back_shift(wm, w.inv_depth), s0, np.ones(w.L, bool)))
            d = tri_ref.window_triangulation(wm, "all", stereo=stereo)["depth"]
            worst["a"] = [max(worst["a"][0], _rel(d, r["depth"], st)), max(worst["a"][1], _rel(d, r["depth"], ~st))]
        # the feature windows see stereo = 0 as first observations without a right camera
        ws = w
        if not stereo:
            ws = w.twin()
            ws.obs_is_stereo = w.obs_is_stereo.copy()
            ws.obs_is_stereo[w.lm_obs_offset[:-1]] = 0
        d = fw_triangulate(ws, host_lib, "vilo_fw_")
        worst["c"] = [max(worst["c"][0], _rel(d, r["depth"], st)), max(worst["c"][1], _rel(d, r["depth"], ~st))]
        if ref_lib is not None:
            with ref_globals(ref_lib, 1 if stereo else 0):
                d = fw_triangulate(w, ref_lib, "ref_fm_")
            worst["b"] = [max(worst["b"][0], _rel(d, r["depth"], st)), max(worst["b"][1], _rel(d, r["depth"], ~st))]
            s = fw_back_shift(w, w.inv_depth, ref_lib, "ref_fm_")
            ok = np.isfinite(s)
            shift = max(shift, _rel(tri_ref.back_shift(w, w.inv_depth), s, ok))
    print("MEASURED floor |d depth| / depth: stereo (a) %.1e (b) %.1e (c) %.1e; two-frame (a) %.1e (b) %.1e (c) %.1e; back-shift (a, b) %.1e"
          % (worst["a"][0], worst["b"][0], worst["c"][0], worst["a"][1], worst["b"][1], worst["c"][1], shift))
    assert max(v[0] for v in worst.values()) <= tri_ref.FLOOR_STEREO
    assert max(v[1] for v in worst.values()) <= tri_ref.FLOOR_TWO_FRAME
    assert shift <= tri_ref.FLOOR_SHIFT
    assert tri_ref.TOL_STEREO == 10 * tri_ref.FLOOR_STEREO and tri_ref.TOL_TWO_FRAME == 10 * tri_ref.FLOOR_TWO_FRAME


@pytest.mark.skipif(not os.path.exists(REF), reason="needs libref.so (the reference tree compiled by build())")
@pytest.mark.parametrize("seed", [0, 1])
def test_tri_ref_matches_the_compiled_reference(seed):
    """Random windows through the reference's own FeatureManager: the stereo branch, the two-frame branch, the INIT_DEPTH fallback (for
    two values of INIT_DEPTH) and removeBackShiftDepth, both of its outcomes."""
    from cerberus_amd import synth
    from oracle import oracle_py as O
    cfg = synth.default_config()
    lib = C.CDLL(REF)
    base = _window(cfg, O.config_from(cfg), seed=900 + seed, L=60 + 7 * seed, prior=False)
    w, mir = mirrored(third_mono(base))
    for stereo, init_depth in ((1, 5.0), (0, 5.0), (1, 2.5)):
        r = tri_ref.window_triangulation(w, "all", stereo=bool(stereo), init_depth=init_depth, write=True)
        assert (np.abs(r["z"]) > Z_CLEAR).all()
        with ref_globals(lib, stereo, init_depth):
            d = fw_triangulate(w, lib, "ref_fm_")
            s = fw_back_shift(w, r["inv_depth"], lib, "ref_fm_")
        st = (r["flags"] & STE) != 0
        fall = (r["flags"] & FALL) != 0
        # (at the generator's perturbed poses some two-frame landmarks come out behind the camera of themselves: low parallax)
        assert (~fall & st).any() == bool(stereo) and (~fall & ~st).any() and set(mir) <= set(np.flatnonzero(fall))
        np.testing.assert_array_equal(d[fall], init_depth)
        assert _rel(d, r["depth"], st) <= tri_ref.FLOOR_STEREO and _rel(d, r["depth"], ~st) <= tri_ref.FLOOR_TWO_FRAME
        assert _rel(r["shift_inv_depth"], s, np.isfinite(s)) <= tri_ref.FLOOR_SHIFT
    # the back-shift's own fallback: a negative depth on a frame-0 landmark lands behind frame 1's camera
    lam = w.inv_depth.copy()
    neg = np.flatnonzero(w.lm_start_frame == 0)[:3]
    lam[neg] = -0.5
    with ref_globals(lib, 1, 2.5):
        s = fw_back_shift(w, lam, lib, "ref_fm_")
    ours = tri_ref.back_shift(w, lam, 2.5)
    np.testing.assert_array_equal(ours[neg], 1.0 / 2.5)
    assert _rel(ours, s, np.isfinite(s)) <= tri_ref.FLOOR_SHIFT
    other = w.lm_start_frame != 0
    np.testing.assert_array_equal(ours[other], lam[other])


def test_selection_and_write_of_the_definition():
    w = shape_window("L70").twin()
    w.inv_depth[[2, 5, 11]] = -1.0
    r = tri_ref.window_triangulation(w, "unset", write=True)
    assert list(np.flatnonzero(r["flags"] & SEL)) == [2, 5, 11]
    rest = np.ones(w.L, bool); rest[[2, 5, 11]] = False
    np.testing.assert_array_equal(r["depth"][rest], 1.0 / w.inv_depth[rest])
    np.testing.assert_array_equal(r["inv_depth"][rest], w.inv_depth[rest])
    np.testing.assert_array_equal(r["inv_depth"][~rest], 1.0 / r["depth"][~rest])
    m = np.zeros(w.L, np.uint8); m[::7] = 1
    r = tri_ref.window_triangulation(w, "mask", mask=m)
    np.testing.assert_array_equal((r["flags"] & SEL) != 0, m != 0)
    np.testing.assert_array_equal(r["inv_depth"], w.inv_depth)


def test_wrapper_options_need_no_device():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    assert C.sizeof(T.TriangulateOpts) == 24
    o, m = api.triangulate_opts(5)
    assert (o.init_depth, o.stereo, o.select, o.write) == (5.0, 1, 0, 0) and m is None
    o, m = api.triangulate_opts(3, select="mask", mask=[0, 2, 0], write=True, init_depth=2.5, stereo=False)
    assert (o.init_depth, o.stereo, o.select, o.write) == (2.5, 0, 2, 1)
    assert m.dtype == np.uint8 and list(m) == [0, 1, 0] and m.flags["C_CONTIGUOUS"]
    assert api.triangulate_opts(0, select="all")[0].select == 1
    for kw in (dict(select="every"), dict(select="mask"), dict(select="all", mask=[1, 1, 1]), dict(select="mask", mask=[1, 1]),
               dict(init_depth=-1.0), dict(init_depth=0.0), dict(init_depth=float("nan")), dict(init_depth=float("inf"))):
        with pytest.raises(ValueError):
            api.triangulate_opts(3, **kw)
    assert api.Triangulation._fields == ("depth", "flags", "offsets", "shift_inv_depth")
    # the header's struct and the mirror agree field by field
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    body = hdr[hdr.index("typedef struct {\n  double init_depth;"):hdr.index("} vilo_triangulate_opts;")]
    assert [f for f, _ in T.TriangulateOpts._fields_] == [ln.split(";")[0].split()[-1] for ln in body.splitlines()[1:] if ";" in ln]
