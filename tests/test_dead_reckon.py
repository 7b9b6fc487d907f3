"""CPU: the numpy definition of vilo_batch_dead_reckon (tests/deadreckon_ref.py): the measured FP64 floor that sets the GPU tolerance
(deadreckon_ref.TOL = 10 x deadreckon_ref.FLOOR), the tie to the oracle's preintegration record (which is pinned against the
reference's own source), what the parity inputs would catch, the statuses of the definition, the option parsing of the Python wrapper,
the struct sizes, the library's exports and the stand-alone sanitizer check of the host half (tests/host_check/dead_reckon_check.cpp).
tests/test_dead_reckon_gpu.py takes its cases from here."""
import ctypes as C
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import alt_config
import deadreckon_ref as D
from conftest import ROOT
from test_gyro_align import kind_window, solved_kind_window

RANGES = (0, 1, 2, 30)   # samples of a range: no step twice over, one step, and the longest range any test uses (the floor is taken there)
WRONG = ("no_g", "R_transposed", "gyr_end", "swap_biases")


def g_norms():
    from cerberus_amd import synth
    cfg = synth.default_config()
    return cfg.g_norm, alt_config.alt_config(cfg).g_norm


@functools.lru_cache(maxsize=None)
def frames_window(F):
    """the first F frames of the 70-landmark window"""
    from test_gpu_parity import _truncate
    w = kind_window("L70", 1).twin()
    w.prior = w.prior.copy()   # (_truncate switches the prior off in place: not the cached window's)
    return _truncate(w, F)


def explicit_frame(w):
    """the explicit from_frame of the parity cases: the frame before the window's last (frame f + 1 exists: write has a target)"""
    return w.F - 2


def take(w, n, first):
    """n consecutive rows of the window's sample array from row `first` on, [n, 35]"""
    assert first + n <= len(w.samples)
    return w.samples[first:first + n]


def batch_ranges(ws, shift=0):
    """(samples [sum n, 35], offsets [W + 1]) of a batch: window i reads RANGES[(i + shift) % 4] rows of its own sample array from row
    3 i + shift on, so that ranges of 0, 1, 2 and 30 samples sit side by side and twins of one window read different rows"""
    parts, off = [], [0]
    for i, w in enumerate(ws):
        n = RANGES[(i + shift) % len(RANGES)]
        parts.append(take(w, n, 3 * (i % 16) + shift))
        off.append(off[-1] + n)
    return np.ascontiguousarray(np.concatenate(parts)), np.array(off, np.int32)


def parity_windows(solved):
    """(tag, window) of the GPU parity test: 11 frames with leg and with IMU-only factors, 6 frames; 3 and 2 frames at the initial state
    only (two or three frames without a prior are no problem to solve). solved: after the oracle's 4-iteration solve, the CPU stand-in
    for the state the device reaches (the two agree to 1e-8)."""
    get = solved_kind_window if solved else kind_window
    out = [("L9 use_leg 1", get("L9", 1)), ("L9 use_leg 0", get("L9", 0)), ("F6", get("F6", 1))]
    if not solved:
        out += [("F3", frames_window(3)), ("F2", frames_window(2))]
    return out


def parity_cases():
    """(tag, window, samples [n, 35], from_frame) of every case the GPU parity test compares"""
    out = []
    for state, solved in (("initial", False), ("solved", True)):
        for i, (name, w) in enumerate(parity_windows(solved)):
            for n in RANGES:
                for f in (-1, explicit_frame(w)):
                    out.append(("%s %s, %d samples, from_frame %d" % (name, state, n, f), w, take(w, n, 3 * i), f))
    return out


def _ulp_moved(w, samples, rng):
    """the window and the samples with every start-state value and every sample value moved by one unit in the last place, up or down"""
    t = w.twin()
    s = samples.copy()
    for a in (t.pose, t.speed_bias, s):
        a[...] = np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))
    return t, s


def test_fp64_floor_measured():
    """Prints the floor of the definition over the parity cases at both g_norm: (a) one unit in the last place on every start-state and
    sample value, (b) the recurrence in numpy.longdouble rounded at the end. deadreckon_ref.FLOOR must cover the larger; the largest
    values come from the 30-sample ranges, the longest any test uses (rounding grows with the number of steps)."""
    rng = np.random.default_rng(23)
    wa, wb = np.zeros(3), np.zeros(3)
    longest = 0.0
    for g in g_norms():
        for tag, w, s, f in parity_cases():
            r = D.window_dead_reckon(w, s, g, f)
            assert r.status == D.OK and r.n_steps == max(0, len(s) - 1), tag
            assert r.n_steps == 0 or r.trajectory[-1].tobytes() == r.state.tobytes(), tag
            worst = 0.0
            for _ in range(4):
                t, sm = _ulp_moved(w, s, rng)
                e = D.state_errors(D.window_dead_reckon(t, sm, g, f).state, r.state)
                wa = np.maximum(wa, e)
                worst = max(worst, max(e))
            e = D.state_errors(D.window_dead_reckon(w, s, g, f, dtype=np.longdouble).state, r.state)
            wb = np.maximum(wb, e)
            if len(s) == max(RANGES):
                longest = max(longest, worst, max(e))
    print("MEASURED floor: (a) P %.1e V %.1e R %.1e; (b) P %.1e V %.1e R %.1e; at %d samples %.1e"
          % (wa[0], wa[1], wa[2], wb[0], wb[1], wb[2], max(RANGES), longest))
    assert np.finfo(np.longdouble).eps < 1e-18   # (b) is a second route only where long double is wider than double
    assert max(wa.max(), wb.max()) <= D.FLOOR
    assert longest == max(wa.max(), wb.max())
    assert D.TOL == 10 * D.FLOOR


def _record_state(w, k, g_norm, leg):
    """the state the oracle's record of interval k - 1 composes from frame k - 1: P_i + V_i T - 1/2 g T^2 + R_i dp, R_i R(dq), V_i - g T +
    R_i dv (the residual of IMUFactor / IMULegFactor set to zero), and the record's linearisation point (ba, bg)"""
    rec = w.preint[k - 1] if leg else w.preint_imu[k - 1]
    T, dp, dq, dv = rec[0], rec[1:4], rec[4:8], rec[8:11]
    lin = rec[23:29] if leg else rec[11:17]
    Ri = D.quat_R(D.quat_normalized(w.pose[k - 1, 3:7]))
    g = np.array([0.0, 0.0, g_norm])
    P = w.pose[k - 1, 0:3] + w.speed_bias[k - 1, 0:3] * T - 0.5 * g * T * T + Ri @ dp
    V = w.speed_bias[k - 1, 0:3] - g * T + Ri @ dv
    return np.concatenate([P, D.quat_from_R(Ri @ D.quat_R(dq)), V]), lin


def test_tie_to_the_pinned_preintegration():
    """The window's own samples of interval k - 1 from frame k - 1, the state's biases at the record's linearisation point, against the
    state composed from the oracle's preintegration record (pinned against the reference's sources by tests/test_oracle_vs_reference.py).
    The two are not the same arithmetic: the record chains a normalised quaternion in the body frame, the dead reckoning an un-normalised
    matrix in the world frame. Their difference is measured here (deadreckon_ref.RECORD_DIFF) and gated at twice that value; the
    bound a wrong recurrence would have to slip under is the sensitivity test's."""
    worst, worst_short = 0.0, 0.0
    for g in g_norms():
        for name, leg in (("L9", 1), ("L70", 1), ("F6", 1), ("L9", 0)):
            w = kind_window(name, leg)
            for k in range(1, w.F):
                ref, lin = _record_state(w, k, g, leg)
                t = w.twin()
                t.speed_bias[k - 1, 3:9] = lin
                s = w.samples[w.sample_offsets[k - 1]:w.sample_offsets[k]]
                r = D.window_dead_reckon(t, s, g, k - 1)
                assert r.status == D.OK and r.n_steps == len(s) - 1 > 0
                e = D.state_error(r.state, ref)
                worst = max(worst, e)
                th = np.abs(s[1:, 4:7] * s[1:, 0:1]).max()
                worst_short = max(worst_short, th ** 3 * r.n_steps)
    print("MEASURED difference to the record-composed state: %.1e (gate %.0e); |gyr dt|^3 n_steps up to %.1e" % (worst, 2 * D.RECORD_DIFF, worst_short))
    assert worst <= 2 * D.RECORD_DIFF
    assert worst >= 0.25 * D.RECORD_DIFF   # (the constant is what is measured, not a loose cover)


@pytest.mark.parametrize("which", ["default", "alt"])
def test_the_parity_inputs_catch_a_wrong_recurrence(which):
    """dropping g, transposing R, taking the end-point gyro sample for the mid-point, swapping ba and bg: each moves the result of every
    parity case that makes a step by at least 1000 x TOL"""
    g = g_norms()[which == "alt"]
    least = {k: np.inf for k in WRONG}
    n = 0
    for tag, w, s, f in parity_cases():
        if len(s) < 2:
            continue
        n += 1
        r = D.window_dead_reckon(w, s, g, f)
        for k in WRONG:
            e = D.state_error(D.window_dead_reckon(w, s, g, f, wrong=k).state, r.state)
            least[k] = min(least[k], e)
            assert e >= 1000 * D.TOL, (tag, k, e)
    assert n > 0
    print("MEASURED smallest change (g_norm %.3f): %s; 1000 x TOL = %.0e" % (g, ", ".join("%s %.1e" % kv for kv in least.items()), 1000 * D.TOL))
    # the other g_norm is told from this one by the same margin
    other = g_norms()[which != "alt"]
    for tag, w, s, f in parity_cases():
        if len(s) >= 2:
            assert D.state_error(D.window_dead_reckon(w, s, other, f).state, D.window_dead_reckon(w, s, g, f).state) >= 1000 * D.TOL, tag


def test_statuses_of_the_definition():
    g = g_norms()[0]
    w = kind_window("L9", 1)
    two = frames_window(2)
    s = take(w, 30, 0)
    for n in (0, 1):
        r = D.window_dead_reckon(w, s[:n], g)
        f = w.F - 1
        want = np.concatenate([w.pose[f, :3], D.quat_from_R(D.quat_R(D.quat_normalized(w.pose[f, 3:7]))), w.speed_bias[f, :3]])
        assert (r.status, r.n_steps) == (D.OK, 0) and r.trajectory.shape == (0, 10) and r.state.tobytes() == want.tobytes()
    assert D.window_dead_reckon(two, s, g, 5).status == D.NO_FRAME
    assert D.window_dead_reckon(two, s, g, 1).status == D.OK and D.window_dead_reckon(two, s, g, 1, write=True).status == D.NO_FRAME
    r = D.window_dead_reckon(two, s, g, 1, write=True)
    assert r.n_steps == 29 and not r.state.any() and r.trajectory.shape == (29, 10) and not r.trajectory.any()
    bad = w.twin()
    bad.speed_bias[w.F - 1, 1] = np.nan
    r = D.window_dead_reckon(bad, s, g)
    assert r.status == D.NUMERIC and not r.state.any() and not r.trajectory.any() and r.n_steps == 29
    assert D.window_dead_reckon(bad, s, g, 3).status == D.OK   # (another frame's velocity)
    sn = s.copy()
    sn[7, 5] = np.inf
    assert D.window_dead_reckon(w, sn, g).status == D.NUMERIC
    sn = s.copy()
    sn[0, 0] = np.nan   # the first sample's dt is not read
    assert D.window_dead_reckon(w, sn, g).state.tobytes() == D.window_dead_reckon(w, s, g).state.tobytes()
    sn[0, 7] = np.nan   # nor is anything but dt, acc, gyr
    assert D.window_dead_reckon(w, sn, g).status == D.OK


def test_quaternion_of_every_branch():
    """Quaterniond(Matrix3d): the trace branch and the three others give the rotation back"""
    rng = np.random.default_rng(3)
    seen = set()
    for q in [[1.0, 0.02, 0.01, 0.03], [0.01, 1.0, -0.02, 0.02], [0.02, 0.01, 1.0, -0.03], [0.5, 0.5, 0.5, 0.5]] + [rng.normal(size=4) for _ in range(40)]:
        q = D.quat_normalized(np.asarray(q, float))
        R = D.quat_R(q)
        t = np.trace(R)
        seen.add(3 if t > 0 else int(np.argmax(np.diag(R))))
        p = D.quat_from_R(R)
        assert min(np.abs(p - q).max(), np.abs(p + q).max()) <= 1e-15
    assert seen == {0, 1, 2, 3}


def test_wrapper_options_need_no_device():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    o = api.dead_reckon_opts()
    assert (o.from_frame, o.write) == (-1, 0)
    o = api.dead_reckon_opts(3, True)
    assert (o.from_frame, o.write) == (3, 1)
    assert api.dead_reckon_opts(T.MAX_FRAMES - 1).from_frame == T.MAX_FRAMES - 1 and api.dead_reckon_opts(0, True).from_frame == 0
    for bad in (dict(from_frame=-2), dict(from_frame=T.MAX_FRAMES), dict(from_frame=1.5), dict(write=True), dict(from_frame=-1, write=True)):
        with pytest.raises(ValueError):
            api.dead_reckon_opts(**bad)
    assert api.DeadReckoning._fields == ("state", "trajectory", "step_offsets", "n_steps", "status")
    assert (T.DR_OK, T.DR_NO_FRAME, T.DR_NUMERIC) == (D.OK, D.NO_FRAME, D.NUMERIC) and T.DR_STATE == 10
    assert hasattr(api.Batch, "dead_reckon") and hasattr(api.Context, "window_dead_reckon")


def _header_struct(name):
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    end = hdr.index("} %s;" % name)
    body = hdr[hdr.rindex("typedef struct {", 0, end):end]
    return [ln.split(";")[0].split() for ln in body.splitlines()[1:] if ";" in ln]


def test_struct_sizes_match_the_header():
    from cerberus_amd import _ctypes as T
    for name, mirror in (("vilo_dead_reckon_opts", T.DeadReckonOpts), ("vilo_window_dead_reckon_record", T.WindowDeadReckonRecord)):
        fields = _header_struct(name)
        assert [f for f, _ in mirror._fields_] == [f[-1] for f in fields] and all(f[0] == "int32_t" for f in fields)
        assert C.sizeof(mirror) == 4 * len(fields) == 8
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    for k, v in (("OK", 0), ("NO_FRAME", 1), ("NUMERIC", 2)):
        assert re.search(r"#define VILO_DR_%s %d\b" % (k, v), hdr), k
    # the columns deadreckon_ref reads of a sample row are the header's dt, acc, gyr
    assert [n for n, _ in T.Sample._fields_][:3] == ["dt", "acc", "gyr"] and T.Sample.acc.offset == 8 and T.Sample.gyr.offset == 32


def test_library_exports_the_entry_points():
    from cerberus_amd import _ctypes as T
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for name in ("vilo_default_dead_reckon_opts", "vilo_batch_dead_reckon", "vilo_window_dead_reckon", "vilo_last_dead_reckon_ms"):
        assert hasattr(lib, name), name
    o = T.DeadReckonOpts(7, 7)
    lib.vilo_default_dead_reckon_opts(C.byref(o))   # host code: needs no device
    assert (o.from_frame, o.write) == (-1, 0)


def test_host_half_under_sanitizers(tmp_path):
    """tests/host_check/dead_reckon_check.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers: the
    argument checks, the step offsets and the packing of cerberus_amd/csrc/deadreckon_host.hpp on a CPU"""
    exe = str(tmp_path / "dead_reckon_check")
    src = os.path.join(ROOT, "tests", "host_check", "dead_reckon_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                   check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip() == "ok", p.stdout
