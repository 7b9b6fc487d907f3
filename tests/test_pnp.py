"""CPU: the numpy definition of vilo_batch_frame_pose_pnp (tests/pnp_ref.py): the measured FP64 floor that sets the GPU tolerances
(pnp_ref.TOL_* = 10 x pnp_ref.FLOOR_*), stationarity of its result, the option parsing of the Python wrapper, the struct
sizes and the library's exports. tests/test_pnp_gpu.py takes its cases from here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import pnp_ref
from conftest import ROOT
from test_triangulate import SHAPES, shape_window, solved_window

# frames of a case: the window's last frame and frame 2. (L9 has 2 usable points on frame 1 and 4 on frame 2.)
FRAMES = (-1, 2)


def cases():
    """(tag, window, frame) of every case: the four packing shapes at the initial state and at the oracle's 4-iteration solved state.
    Every one of them converges within the call's cap of 20 steps (asserted in test_reference_converges_and_is_stationary): none dropped."""
    out = []
    for name in SHAPES:
        for state, w in (("initial", shape_window(name)), ("solved", solved_window(name))):
            out += [("%s %s frame %d" % (name, state, f), w, f) for f in FRAMES]
    return out


def _ulp_moved(w, rng):
    """the window with every pose / extrinsic entry, inverse depth and observation coordinate moved by one unit in the last place"""
    t = w.twin()
    t.obs = w.obs.copy()
    for a in (t.pose, t.ex_pose, t.inv_depth, t.obs):
        a[...] = np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
    return t


def test_fp64_floor_measured():
    """Prints the floor of the definition over the cases: (a) one unit in the last place on everything the minimiser reads, (b) the
    left-perturbation / normal-equation minimiser against the right-perturbation / lstsq one. pnp_ref.FLOOR_* must cover the larger.
    Measured (x86-64, numpy's LAPACK): position (a) 2.3e-15 (b) 2.3e-15, rotation (a) 4.9e-16 (b) 3.3e-16."""
    rng = np.random.default_rng(7)
    worst = {"a": [0.0, 0.0], "b": [0.0, 0.0]}
    for tag, w, f in cases():
        r = pnp_ref.frame_pose(w, f)
        assert r.status == pnp_ref.OK, tag
        for _ in range(3):
            m = pnp_ref.frame_pose(_ulp_moved(w, rng), f)
            assert m.status == pnp_ref.OK, tag
            e = pnp_ref.rigid_errors(m.R, m.P, r.R, r.P)
            worst["a"] = [max(worst["a"][0], e[0]), max(worst["a"][1], e[1])]
        e = pnp_ref.rigid_errors(*pnp_ref.frame_pose_right(w, f), r.R, r.P)
        worst["b"] = [max(worst["b"][0], e[0]), max(worst["b"][1], e[1])]
    print("MEASURED floor: position (a) %.1e (b) %.1e; rotation (a) %.1e (b) %.1e" % (worst["a"][0], worst["b"][0], worst["a"][1], worst["b"][1]))
    assert max(v[0] for v in worst.values()) <= pnp_ref.FLOOR_POS
    assert max(v[1] for v in worst.values()) <= pnp_ref.FLOOR_ROT
    assert pnp_ref.TOL_POS == 10 * pnp_ref.FLOOR_POS and pnp_ref.TOL_ROT == 10 * pnp_ref.FLOOR_ROT


@pytest.mark.parametrize("guess", ["previous", "current"])
def test_reference_converges_and_is_stationary(guess):
    for tag, w, f in cases():
        r = pnp_ref.frame_pose(w, f, guess)
        assert r.status == pnp_ref.OK and r.n_points >= 4, tag
        assert np.abs(r.g).max() <= pnp_ref.STATIONARY * max(1.0, np.abs(r.H).max()), (tag, np.abs(r.g).max())
        # Gauss-Newton converges linearly here (the reprojection residual is not zero: each step is 30 to 100 times shorter than the one
        # before), so the stop rule leaves a truncation error of its own beside the arithmetic one the floor measures. At the call's
        # default step_tolerance of 1e-12 it is below the tolerance itself (rate < 1/2: less than the last step); the GPU parity test asks
        # for PARITY_STEP_TOLERANCE, where it is inside the GPU tolerance — both within the cap of 20 steps.
        d = pnp_ref.frame_pose(w, f, guess, max_iterations=20, step_tolerance=1e-12)
        c = pnp_ref.frame_pose(w, f, guess, max_iterations=20, step_tolerance=pnp_ref.PARITY_STEP_TOLERANCE)
        assert d.status == pnp_ref.OK and c.status == pnp_ref.OK and d.iterations <= c.iterations <= 20, (tag, d.iterations, c.iterations)
        dp, dr = pnp_ref.rigid_errors(d.R, d.P, r.R, r.P)
        ep, er = pnp_ref.rigid_errors(c.R, c.P, r.R, r.P)
        print("MEASURED %s %s: steps %d / %d / %d (reference / default / parity); default stop leaves %.1e, %.1e; parity stop %.1e, %.1e"
              % (tag, guess, r.iterations, d.iterations, c.iterations, dp, dr, ep, er))
        assert dp <= 1e-12 and dr <= 1e-12, (tag, dp, dr)
        assert ep <= pnp_ref.TOL_POS and er <= pnp_ref.TOL_ROT, (tag, ep, er)
        assert r.final_cost <= r.initial_cost
        assert r.pose[6] >= 0 and abs(np.linalg.norm(r.pose[3:7]) - 1.0) < 1e-15


def test_selection_of_the_definition():
    w = shape_window("L9")
    assert len(pnp_ref.points(w, 1)[2]) == 2 and len(pnp_ref.points(w, 2)[2]) == 4
    assert pnp_ref.frame_pose(w, 1).status == pnp_ref.NOT_ENOUGH_POINTS
    np.testing.assert_array_equal(pnp_ref.frame_pose(w, 1).pose, w.pose[1])
    f6 = shape_window("F6")
    assert pnp_ref.frame_pose(f6, 6).status == pnp_ref.NO_FRAME and pnp_ref.frame_pose(f6, 5).status == pnp_ref.OK
    # a landmark that starts on the frame, or has no depth, is not used
    w70 = shape_window("L70").twin()
    k = w70.F - 1
    ids = pnp_ref.points(w70, k)[2]
    assert (w70.lm_start_frame[ids] < k).all()
    w70.inv_depth[ids[:3]] = -1.0
    assert list(pnp_ref.points(w70, k)[2]) == list(ids[3:])


def test_wrapper_options_need_no_device():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    o = api.pnp_opts()
    assert (o.frame, o.guess, o.write, o.max_iterations, o.step_tolerance) == (-1, 0, 0, 20, 1e-12)
    o = api.pnp_opts(frame=10, guess="current", write=True, max_iterations=64, step_tolerance=0.0)
    assert (o.frame, o.guess, o.write, o.max_iterations, o.step_tolerance) == (10, 1, 1, 64, 0.0)
    assert api.pnp_opts(frame=1, max_iterations=1).frame == 1
    for kw in (dict(guess="next"), dict(frame=-2), dict(frame=0), dict(frame=11), dict(frame=1.5), dict(max_iterations=0),
               dict(max_iterations=65), dict(step_tolerance=-1e-3), dict(step_tolerance=float("nan")), dict(step_tolerance=float("inf"))):
        with pytest.raises(ValueError):
            api.pnp_opts(**kw)
    assert api.FramePose._fields == ("pose", "final_cost", "initial_cost", "n_points", "iterations", "status")
    assert (T.PNP_OK, T.PNP_NOT_ENOUGH_POINTS, T.PNP_NO_CONVERGENCE, T.PNP_NUMERIC, T.PNP_NO_FRAME) == \
        (pnp_ref.OK, pnp_ref.NOT_ENOUGH_POINTS, pnp_ref.NO_CONVERGENCE, pnp_ref.NUMERIC, pnp_ref.NO_FRAME)


def _header_struct(name):
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    end = hdr.index("} %s;" % name)
    body = hdr[hdr.rindex("typedef struct {", 0, end):end]
    return [ln.split(";")[0].split() for ln in body.splitlines()[1:] if ";" in ln]


def test_struct_sizes_match_the_header():
    from cerberus_amd import _ctypes as T
    size = {"int32_t": 4, "double": 8}
    for name, mirror, want in (("vilo_pnp_opts", T.PnpOpts, None), ("vilo_window_pnp_record", T.WindowPnpRecord, 32)):
        fields = _header_struct(name)
        assert [f for f, _ in mirror._fields_] == [f[-1] for f in fields]
        assert [C.sizeof(t) for _, t in mirror._fields_] == [size[f[0]] for f in fields]
        hdr_size = sum(size[f[0]] for f in fields)   # (fields in descending alignment or paired: no padding beyond the named pad)
        assert C.sizeof(mirror) == hdr_size and (want is None or hdr_size == want)
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    for k, v in (("GUESS_PREVIOUS", 0), ("GUESS_CURRENT", 1), ("OK", 0), ("NOT_ENOUGH_POINTS", 1), ("NO_CONVERGENCE", 2), ("NUMERIC", 3),
                 ("NO_FRAME", 4)):
        assert re.search(r"#define VILO_PNP_%s %d\b" % (k, v), hdr), k
    assert T.MAX_FRAMES == int(re.search(r"#define VILO_MAX_FRAMES (\d+)", hdr).group(1))


def test_library_exports_the_entry_points():
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for name in ("vilo_default_pnp_opts", "vilo_batch_frame_pose_pnp", "vilo_window_frame_pose_pnp", "vilo_last_pnp_ms"):
        assert hasattr(lib, name), name
    from cerberus_amd import _ctypes as T
    o = T.PnpOpts()
    lib.vilo_default_pnp_opts(C.byref(o))   # host code: needs no device
    assert (o.frame, o.guess, o.write, o.max_iterations, o.step_tolerance) == (-1, 0, 0, 20, 1e-12)
