"""CPU: the numpy definition of vilo_batch_dead_reckon_covariance (tests/drcov_ref.py): the measured FP64 floor that sets the GPU tolerance
(drcov_ref.TOL = 10 x drcov_ref.FLOOR), what the parity inputs would catch of a wrong recurrence at both configurations,
the tie to the oracle's IMU preintegration covariance (which is pinned against the reference's own source), the no-step and NaN rules of
the definition, the option parsing and the cov_in helper of the Python wrapper, the struct sizes, the library's exports and the
stand-alone sanitizer check of the host half (tests/host_check/dr_cov_check.cpp). tests/test_dr_covariance_gpu.py takes its cases from
here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import alt_config
import deadreckon_ref as D
import drcov_ref as DC
from conftest import ROOT
from test_dead_reckon import RANGES, explicit_frame, frames_window
from test_gyro_align import kind_window, solved_kind_window

DT_SCALE = np.array([1.0, 0.6, 1.4, 0.8, 1.2, 0.5, 1.5])   # unequal dt inside a range


def take(w, n, first):
    """n consecutive rows of the window's sample array from row `first` on, [n, 35], with dt made unequal from row to row"""
    assert first + n <= len(w.samples)
    s = w.samples[first:first + n].copy()
    s[:, 0] *= DT_SCALE[np.arange(n) % len(DT_SCALE)]
    return s


def configs():
    """(g_norm, noise) at the default configuration and at tests/alt_config.py's"""
    from cerberus_amd import synth
    cfg = synth.default_config()
    alt = alt_config.alt_config(cfg)
    return {"default": (cfg.g_norm, DC.noise_of(cfg)), "alt": (alt.g_norm, DC.noise_of(alt))}


@functools.lru_cache(maxsize=None)
def solved_frames(name, use_leg):
    """the frame blocks [11, 19, 19] of the solved window by the numpy definition of vilo_batch_covariance: the CPU stand-in for what the
    GPU parity test cuts its cov_in from"""
    import cov_ref
    from cerberus_amd import synth
    from oracle import oracle_py as O
    fr, _ = cov_ref.window_covariance(O.config_from(synth.default_config()), solved_kind_window(name, use_leg), gauge="frame0")
    return fr


def given_cov(seed):
    """a covariance that comes from no solve: A A^T of a seeded 15 x 15 A with rows scaled to a frame block's magnitudes (1e-2 m, 1e-2
    rad, 1e-1 m/s, 1e-3 m/s^2, 1e-4 rad/s), for the windows of 2 and 3 frames, which no solve gives one (two or three frames without a
    prior do not separate the accelerometer bias from gravity: vilo_batch_covariance reports them singular)"""
    A = np.random.default_rng(seed).normal(size=(DC.N, DC.N)) * np.repeat([1e-2, 1e-2, 1e-1, 1e-3, 1e-4], 3)[:, None]
    return A @ A.T


def parity_windows():
    """(tag, window, what cov_in is) of the GPU parity test: 11 frames with leg and with IMU-only factors, 6, 3 and 2 frames at the initial
    state with cov_in NULL; the 3- and 2-frame ones also with a given covariance; the 11- and 6-frame ones again after a 4-iteration
    solve with cov_in cut from the solved window's covariance (frames [11, 19, 19])"""
    out = [("L9 use_leg 1 initial", kind_window("L9", 1), None), ("L9 use_leg 0 initial", kind_window("L9", 0), None),
           ("F6 initial", kind_window("F6", 1), None), ("F3 initial", frames_window(3), None), ("F2 initial", frames_window(2), None),
           ("F3 initial, given cov_in", frames_window(3), given_cov(3)), ("F2 initial, given cov_in", frames_window(2), given_cov(2))]
    for name, leg in (("L9", 1), ("L9", 0), ("F6", 1)):
        out.append(("%s use_leg %d solved" % (name, leg), solved_kind_window(name, leg), solved_frames(name, leg)))
    return out


def parity_cases():
    """(tag, window, samples [n, 35], from_frame, cov_in [15, 15] or None) of every case the GPU parity test compares"""
    out = []
    for i, (name, w, cov) in enumerate(parity_windows()):
        for n in RANGES:
            for f in (-1, explicit_frame(w)):
                c = cov if cov is None or cov.ndim == 2 else np.ascontiguousarray(cov[w.F - 1 if f == -1 else f, :DC.N, :DC.N])
                out.append(("%s, %d samples, from_frame %d" % (name, n, f), w, take(w, n, 3 * i), f, c))
    return out


def sees_no_F(wrong, samples, cov_in):
    """cov_in = 0 and one step: F S F^T = F 0 F^T = 0 whatever F is, so a mistake that lies in F alone cannot show there"""
    return wrong in ("F_transposed", "swap_bias_columns") and cov_in is None and len(samples) == 2


def _ulp(a, rng):
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))


def _ulp_moved(w, samples, cov_in, rng):
    """every start-state value, every sample value and every cov_in entry of the triangle that is read moved by one unit in the last place"""
    t = w.twin()
    s = samples.copy()
    for a in (t.pose, t.speed_bias, s):
        a[...] = _ulp(a, rng)
    return t, s, None if cov_in is None else _ulp(cov_in, rng)


def test_fp64_floor_measured():
    """Prints the floor of the definition over the parity cases at both configurations: (a) one unit in the last place on every input, (b)
    the recurrence in numpy.longdouble rounded at the end. drcov_ref.FLOOR must cover the larger; it is taken at the longest range."""
    rng = np.random.default_rng(29)
    assert np.finfo(np.longdouble).eps < 1e-18   # (b) is a second route only where long double is wider than double
    wa = wb = longest = 0.0
    for which, (g, noise) in configs().items():
        for tag, w, s, f, c in parity_cases():
            r = DC.window_dr_cov(w, s, g, noise, f, c)
            assert r.status == DC.OK and r.n_steps == max(0, len(s) - 1), tag
            assert r.state.tobytes() == D.window_dead_reckon(w, s, g, f).state.tobytes(), tag
            assert r.cov.tobytes() == r.cov.T.tobytes(), tag
            a = 0.0
            for _ in range(4):
                t, sm, cm = _ulp_moved(w, s, c, rng)
                m = DC.window_dr_cov(t, sm, g, noise, f, cm)
                a = max(a, DC.cov_error(m.cov, r.cov), DC.rows_error(m.pose_cov_trajectory, r.pose_cov_trajectory))
            x = DC.window_dr_cov(w, s, g, noise, f, c, dtype=np.longdouble)
            b = max(DC.cov_error(x.cov, r.cov), DC.rows_error(x.pose_cov_trajectory, r.pose_cov_trajectory))
            wa, wb = max(wa, a), max(wb, b)
            if len(s) == max(RANGES):
                longest = max(longest, a, b)
            print("MEASURED %s %s: (a) %.1e (b) %.1e" % (which, tag, a, b))
    print("MEASURED floor: (a) %.1e (b) %.1e; at %d samples %.1e (FLOOR %.0e)" % (wa, wb, max(RANGES), longest, DC.FLOOR))
    assert longest <= DC.FLOOR
    assert DC.FLOOR <= 10 * longest   # (rounded up, not a loose cover)
    assert DC.TOL == 10 * DC.FLOOR


@pytest.mark.parametrize("which", ["default", "alt"])
def test_the_parity_inputs_catch_a_wrong_recurrence(which):
    """dropping V Q V^T, transposing F, the pre-step R for the post-step R, the ba and bg column blocks swapped, acc_w for gyr_w: each
    moves some entry of every parity case that makes a step by at least 1000 x TOL. One exception, which is arithmetic and not a
    weakness of the inputs: with cov_in NULL the first step computes F 0 F^T = 0 whatever F is, so the two mistakes that lie in F alone
    (the transposition, the swapped columns) change nothing in the one-step cases from zero (sees_no_F; asserted to be exactly nothing).
    The same windows and ranges from a non-zero cov_in, and the 30-sample ranges from zero, do see them."""
    g, noise = configs()[which]
    least = {k: np.inf for k in DC.WRONG}
    n = blind = 0
    for tag, w, s, f, c in parity_cases():
        if len(s) < 2:
            continue
        n += 1
        r = DC.window_dr_cov(w, s, g, noise, f, c)
        for k in DC.WRONG:
            e = DC.cov_error(DC.window_dr_cov(w, s, g, noise, f, c, wrong=k).cov, r.cov)
            if sees_no_F(k, s, c):
                blind += 1
                assert e == 0.0, (tag, k, e)
                continue
            least[k] = min(least[k], e)
            assert e >= 1000 * DC.TOL, (tag, k, e)
    assert blind == 2 * 2 * 5   # two mistakes, two from_frame, the five windows with cov_in NULL
    assert n > 0
    print("MEASURED smallest change (%s): %s; 1000 x TOL = %.0e" % (which, ", ".join("%s %.1e" % kv for kv in least.items()), 1000 * DC.TOL))
    # every noise field is seen: the other configuration's value of one field alone moves every 30-sample case from cov_in = 0, where
    # the noise is all there is, by the same margin. (Against a solved frame's block a bias walk is small: 29 steps add 29 dt^2 w^2, 1e-10
    # and less, to a bias variance of 1e-6 and more, and a factor of 1.45 or 1.7 on w is then below the margin: measured 8.0e-10 on the
    # six-frame window without a prior. The five mistakes above are held on every case.)
    other = configs()["default" if which == "alt" else "alt"][1]
    for field in DC.Noise._fields:
        one = noise._replace(**{field: getattr(other, field)})
        for tag, w, s, f, c in parity_cases():
            if len(s) == max(RANGES) and c is None:
                e = DC.cov_error(DC.window_dr_cov(w, s, g, one, f, c).cov, DC.window_dr_cov(w, s, g, noise, f, c).cov)
                assert e >= 1000 * DC.TOL, (tag, field, e)


def _record(w, k):
    """(covariance [15, 15], lin_ba lin_bg [6]) of the oracle's IMU preintegration record of interval k - 1 (vilo_preint_imu: sum_dt,
    delta_p, delta_q, delta_v, lin_ba, lin_bg, jacobian, covariance)"""
    rec = np.asarray(w.preint_imu[k - 1], float).ravel()
    assert rec.size == 17 + 2 * 225
    return rec[17 + 225:].reshape(15, 15), rec[11:17]


def test_tie_to_the_pinned_preintegration():
    """cov_in = 0, the window's own samples of interval k - 1 from frame k - 1 with the biases at the record's linearisation point:
    cov_out against T S_rec T^T, T = blkdiag(R_0, I, R_0, I, I) (the record's dp and dv are in frame k - 1's body frame, the call's in
    the world frame), S_rec from the oracle's record (pinned against the reference's sources by tests/test_oracle_vs_reference.py).
    With R_0 = I the comparison is against S_rec itself. The two are not the same arithmetic (the record chains a normalised quaternion);
    their difference is measured here (drcov_ref.RECORD_DIFF) and gated at twice that value; it is not rounding."""
    g, noise = configs()["default"]
    worst = worst_identity = 0.0
    for name, leg in (("L9", 1), ("L70", 1), ("F6", 1), ("L9", 0)):
        w = kind_window(name, leg)
        for k in range(1, w.F):
            S_rec, lin = _record(w, k)
            s = w.samples[w.sample_offsets[k - 1]:w.sample_offsets[k]]
            for identity in (False, True):
                t = w.twin()
                t.speed_bias[k - 1, 3:9] = lin
                if identity:
                    t.pose[k - 1, 3:7] = [0.0, 0.0, 0.0, 1.0]
                r = DC.window_dr_cov(t, s, g, noise, k - 1)
                assert r.status == DC.OK and r.n_steps == len(s) - 1 > 0
                R0 = D.quat_R(D.quat_normalized(t.pose[k - 1, 3:7]))
                T = np.eye(15)
                T[0:3, 0:3] = T[6:9, 6:9] = R0
                ref = S_rec if identity else T @ S_rec @ T.T
                e = DC.cov_error(r.cov, ref)
                worst = max(worst, e)
                if identity:
                    worst_identity = max(worst_identity, e)
    print("MEASURED difference to the record's covariance: %.1e (R_0 = I: %.1e; gate %.0e)" % (worst, worst_identity, 2 * DC.RECORD_DIFF))
    assert worst <= 2 * DC.RECORD_DIFF
    assert worst >= 0.25 * DC.RECORD_DIFF   # (the constant is what is measured, not a loose cover)


def test_no_step_returns_the_mirrored_input_and_the_lower_triangle_is_not_read():
    g, noise = configs()["default"]
    w = kind_window("L9", 1)
    rng = np.random.default_rng(5)
    A = rng.normal(size=(15, 15))
    c = A @ A.T
    low = np.tril(np.ones((15, 15), bool), -1)
    poisoned = np.where(low, np.nan, c)
    want = np.triu(c) + np.triu(c, 1).T
    for n in (0, 1):
        for cin in (c, poisoned):
            r = DC.window_dr_cov(w, take(w, n, 0), g, noise, -1, cin)
            assert (r.status, r.n_steps) == (DC.OK, 0) and r.cov.tobytes() == want.tobytes() and r.pose_cov_trajectory.shape == (0, 6, 6)
        r = DC.window_dr_cov(w, take(w, n, 0), g, noise)
        assert r.status == DC.OK and not r.cov.any()
    s = take(w, 30, 0)
    a, b = DC.window_dr_cov(w, s, g, noise, 3, c), DC.window_dr_cov(w, s, g, noise, 3, poisoned)
    assert a.status == b.status == DC.OK and a.cov.tobytes() == b.cov.tobytes()
    assert a.pose_cov_trajectory[-1].tobytes() == a.cov[:6, :6].tobytes() and a.pose_cov_trajectory.shape == (29, 6, 6)
    assert np.linalg.eigvalsh(a.cov).min() >= -DC.FLOOR * np.trace(a.cov)
    # statuses: a NaN in the read triangle, in the start state, in a sample that is read; no such frame
    bad = c.copy()
    bad[2, 7] = np.nan
    r = DC.window_dr_cov(w, s, g, noise, 3, bad)
    assert r.status == DC.NUMERIC and not r.cov.any() and not r.state.any() and not r.pose_cov_trajectory.any() and r.n_steps == 29
    assert DC.window_dr_cov(w, s[:1], g, noise, 3, bad).status == DC.NUMERIC
    t = w.twin()
    t.speed_bias[3, 4] = np.nan
    assert DC.window_dr_cov(t, s, g, noise, 3, c).status == DC.NUMERIC and DC.window_dr_cov(t, s, g, noise, 4, c).status == DC.OK
    sn = s.copy()
    sn[7, 2] = np.inf
    assert DC.window_dr_cov(w, sn, g, noise, 3, c).status == DC.NUMERIC
    assert DC.window_dr_cov(frames_window(2), s, g, noise, 5, bad).status == DC.NO_FRAME


def test_wrapper_options_and_cov_in_helper_need_no_device():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    o = api.dr_cov_opts()
    assert (o.from_frame, o.reserved) == (-1, 0)
    assert api.dr_cov_opts(T.MAX_FRAMES - 1).from_frame == T.MAX_FRAMES - 1 and api.dr_cov_opts(0).from_frame == 0
    for bad in (-2, T.MAX_FRAMES, 1.5):
        with pytest.raises(ValueError):
            api.dr_cov_opts(bad)
    assert api.DeadReckonedCovariance._fields == ("state", "cov", "pose_cov_trajectory", "step_offsets", "n_steps", "status")
    assert (T.DR_COV_N, T.DR_COV_POSE) == (DC.N, DC.POSE)
    assert hasattr(api.Batch, "dead_reckon_covariance") and hasattr(api.Context, "window_dead_reckon_covariance")
    # the helper: the leading 15 x 15 of the chosen frame's block of every window
    rng = np.random.default_rng(2)
    frames = rng.normal(size=(3, T.F, T.COV_FRAME, T.COV_FRAME))
    nf = np.array([11, 2, 6])
    c = api.dr_cov_in(frames, nf)
    assert c.shape == (3, 15, 15) and c.flags["C_CONTIGUOUS"]
    for i, f in enumerate((10, 1, 5)):
        assert c[i].tobytes() == np.ascontiguousarray(frames[i, f, :15, :15]).tobytes()
    c = api.dr_cov_in(frames, nf, 4)
    assert c[0].tobytes() == np.ascontiguousarray(frames[0, 4, :15, :15]).tobytes() and not c[1].any()   # (window 1 has no frame 4)
    assert c[2].tobytes() == np.ascontiguousarray(frames[2, 4, :15, :15]).tobytes()
    for bad in (dict(frames=frames[0]), dict(frames=frames[:, :, :15, :15]), dict(n_frames=nf[:2]), dict(n_frames=[11, 0, 6]),
                dict(n_frames=[11, 12, 6]), dict(n_frames=[11.0, 2.0, 6.0]), dict(from_frame=11), dict(from_frame=-2)):
        kw = dict(frames=frames, n_frames=nf, from_frame=-1)
        kw.update(bad)
        with pytest.raises(ValueError):
            api.dr_cov_in(**kw)


def test_struct_size_and_exports():
    from cerberus_amd import _ctypes as T
    from test_dead_reckon import _header_struct
    fields = _header_struct("vilo_dr_cov_opts")
    assert [f for f, _ in T.DrCovOpts._fields_] == [f[-1] for f in fields] and all(f[0] == "int32_t" for f in fields)
    assert C.sizeof(T.DrCovOpts) == 8
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for name in ("vilo_default_dr_cov_opts", "vilo_batch_dead_reckon_covariance", "vilo_window_dead_reckon_covariance", "vilo_last_dr_cov_ms"):
        assert hasattr(lib, name), name
    o = T.DrCovOpts(7, 7)
    lib.vilo_default_dr_cov_opts(C.byref(o))   # host code: needs no device
    assert (o.from_frame, o.reserved) == (-1, 0)


def test_host_half_under_sanitizers(tmp_path):
    """tests/host_check/dr_cov_check.cpp, a stand-alone program built with the address and undefined-behaviour sanitizers: the argument
    checks, the block sizes and the noise diagonal of cerberus_amd/csrc/drcov_host.hpp, with deadreckon_host.hpp's step offsets and
    packing as the call uses them, at W = 1, an odd shape and W = 32 768, on a CPU"""
    exe = str(tmp_path / "dr_cov_check")
    src = os.path.join(ROOT, "tests", "host_check", "dr_cov_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                   check=True, timeout=300)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip() == "ok", p.stdout
