"""CPU: the option checks of Batch.gauge_fix / Batch.failure_detection that need no device; the numpy definitions (tests/gauge_ref.py)
against the oracle's gauge fix on the 13 Euler-singularity cases of tests/golden/gauge_fix_edges.npz and on random windows; their measured
FP64 floors; that the parity inputs tell the definitions from four plausible mistakes by 1e6 tolerances; that no failure criterion of
the parity inputs sits within 1e-6 of its threshold. The case builders are shared with tests/test_gauge_fix_gpu.py."""
import functools
import os

import numpy as np
import pytest

import gauge_ref as G

GG = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gauge_fix_edges.npz"))
N_GOLDEN = GG["cases"].shape[0]

# name: (landmarks, seed, frames, use_leg, ex_const, generic extrinsic quaternions). F11ex and F11exfree are one window, its extrinsics
# constant and free: the synthetic extrinsic quaternion (0.5, -0.5, 0.5, -0.5) comes back from normalisation, matrix and back with the
# same bits, so a kernel that rewrote a constant block would not show on it. generic_extrinsics() gives them quaternions the rewrite moves.
SHAPES = {"F11": (24, 701, 11, 1, 0, 0), "F11ex": (24, 705, 11, 1, 1, 1), "F11exfree": (24, 705, 11, 1, 0, 1), "F6": (20, 703, 6, 1, 0, 0),
          "F2": (16, 704, 2, 1, 0, 0), "F11imu": (20, 702, 11, 0, 0, 0)}
LEG_GROUP, IMU_GROUP, SOLVED = ("F11", "F11ex", "F11exfree", "F6", "F2"), ("F11imu",), ("F11", "F11ex", "F11exfree", "F6", "F11imu")


def generic_extrinsics(ex_pose):
    """ex_pose [2, 7] with each camera turned by a milliradian about an axis of its own and its quaternion scaled by 1 + 3e-9 and
    1 - 2e-9: as a constant block of a solved estimator looks (Ceres never normalises a constant block), harmless to the factors, and
    far enough from unit length that the normalised rewrite changes its bits whatever the rounding"""
    out = np.array(ex_pose, dtype=np.float64)
    for k, (axis, scale) in enumerate((((0.3, -0.5, 0.8), 1 + 3e-9), ((-0.6, 0.2, 0.7), 1 - 2e-9))):
        ax = np.array(axis) / np.linalg.norm(axis)
        bx, by, bz, bw = np.concatenate([np.sin(5e-4) * ax, [np.cos(5e-4)]])
        x, y, z, s = out[k, 3:7]
        out[k, 3:7] = scale * np.array([s * bx + x * bw + y * bz - z * by, s * by - x * bz + y * bw + z * bx, s * bz + x * by - y * bx + z * bw,
                                        s * bw - x * bx - y * by - z * bz])
    return out


@functools.lru_cache(maxsize=None)
def shape_window(name):
    from cerberus_amd import synth
    from oracle import oracle_py as O
    from test_gpu_parity import _truncate
    L, seed, F, use_leg, ex_const, generic = SHAPES[name]
    cfg = synth.default_config()
    w = synth.make_window(cfg, params=synth.default_params(n_landmarks=L, seed=seed, with_prior=True))
    O.fill_preint(O.config_from(cfg), w)
    if F < 11:
        _truncate(w, F)
    w.ex_const = ex_const
    if generic:
        w.ex_pose[...] = generic_extrinsics(w.ex_pose)
    if not use_leg:
        w.use_leg, w.leg_bias_const = 0, 1
    return w


@functools.lru_cache(maxsize=None)
def solved_window(name, alt=False):
    """after the oracle's 4-iteration solve, at the default configuration or tests/alt_config.py's: the CPU stand-in for the states the
    GPU parity test reaches"""
    import alt_config
    from cerberus_amd import synth
    from oracle import oracle_py as O
    w = shape_window(name).twin()
    cfg = synth.default_config()
    O.solve_window(O.config_from(alt_config.alt_config(cfg) if alt else cfg), w, O.default_opts(True, 4))
    return w


def given_anchor(pose0, k=0):
    """an anchor a yaw of 0.4 + 0.1 k rad, a pitch of 0.1 rad and a metre or two away from a frame-0 pose [7]"""
    y, p = 0.4 + 0.1 * k, 0.1
    qy = np.array([0.0, 0.0, np.sin(y / 2), np.cos(y / 2)])
    qp = np.array([0.0, np.sin(p / 2), 0.0, np.cos(p / 2)])

    def mul(a, b):   # [x y z w]
        ax, ay, az, aw = a
        bx, by, bz, bw = b
        return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by - ax * bz + ay * bw + az * bx, aw * bz + ax * by - ay * bx + az * bw,
                         aw * bw - ax * bx - ay * by - az * bz])
    return np.concatenate([pose0[:3] + np.array([1.0, -2.0, 0.5]), mul(mul(qy, qp), pose0[3:7])])


@functools.lru_cache(maxsize=None)
def golden_windows():
    """[(window at the golden case's solved state, anchor: the case's frame-0 pose before)] of the 13 cases"""
    from cerberus_amd import synth
    from oracle import oracle_py as O
    cfg = synth.default_config()
    base = synth.make_window(cfg, n_landmarks=24, seed=5)
    O.fill_preint(O.config_from(cfg), base)
    out = []
    for n in range(N_GOLDEN):
        w = base.twin()
        w.pose[...], w.speed_bias[...], w.ex_pose[...] = GG["after_pose_%d" % n], GG["after_sb_%d" % n], GG["after_ex_%d" % n]
        out.append((w, GG["before_pose_%d" % n][0].copy()))
    return out


def gauge_case(tag, w, anchor):
    """(tag, anchor [7], pose [F, 7], speed_bias [F, 9], ex_pose [2, 7], ex_const) at the window's state arrays"""
    return (tag, np.array(anchor), w.pose[:w.F].copy(), w.speed_bias[:w.F].copy(), w.ex_pose.copy(), bool(w.ex_const))


def gauge_cases():
    """every case of the GPU parity test, with the oracle's solve standing in for the device's: given anchors at the initial state, uploaded
    and given anchors at the solved states of both configurations, the golden cases with their own anchors"""
    out = []
    for k, name in enumerate(LEG_GROUP + IMU_GROUP):
        w = shape_window(name)
        out.append(gauge_case("%s initial given" % name, w, given_anchor(w.pose[0], k)))
    for alt in (False, True):
        for k, name in enumerate(SOLVED):
            w0, w = shape_window(name), solved_window(name, alt)
            out.append(gauge_case("%s solved%s uploaded" % (name, " alt" * alt), w, w0.pose[0]))
            out.append(gauge_case("%s solved%s given" % (name, " alt" * alt), w, given_anchor(w0.pose[0], k)))
    for n, (w, a) in enumerate(golden_windows()):
        out.append(gauge_case("golden %d pitch %s" % (n, GG["cases"][n]), w, a))
    return out


# last pose of a failure-detection case relative to the last frame's: (translation, rotation angle in degrees about a tilted axis).
#   0 nothing large; 1 everything large; 2 z alone, and an angle that only the reference's 3.14 puts above 50; 3 translation alone
LAST = [((0.3, 0.2, 0.1), 5.0), ((4.0, 3.0, 2.0), 60.0), ((0.0, 0.1, 1.5), 49.99), ((4.0, 3.1, 0.2), 20.0)]
TRACKS = [0, 1, 2, 57]
BIG_BIAS = [None, ((1.5, 1.5, 1.5), (0.01, -0.02, 0.03)), ((0.1, 0.2, -0.1), (0.7, 0.6, 0.5)), ((2.0, -2.0, 1.0), (0.9, 0.9, -0.9))]


def failure_inputs(ws, shift=0):
    """(last_track_num [n], last_pose [n, 7]) of windows at their state arrays: window i gets variant (i + shift) % 4"""
    tracks = np.array([TRACKS[(i + shift) % 4] for i in range(len(ws))], np.int32)
    last = np.zeros((len(ws), 7))
    for i, w in enumerate(ws):
        (t, deg), p = LAST[(i + shift) % 4], w.pose[w.F - 1]
        ax = np.array([0.2, -0.3, 0.9]) / np.linalg.norm([0.2, -0.3, 0.9])
        h = np.radians(deg) / 2
        dq = np.concatenate([np.sin(h) * ax, [np.cos(h)]])
        x, y, z, s = p[3:7]
        bx, by, bz, bw = dq
        last[i, :3] = p[:3] + np.array(t)
        last[i, 3:] = [s * bx + x * bw + y * bz - z * by, s * by - x * bz + y * bw + z * bx, s * bz + x * by - y * bx + z * bw, s * bw - x * bx - y * by - z * bz]
    return tracks, last


def with_big_bias(w, k):
    """a twin of the window whose last frame carries accelerometer / gyroscope biases of BIAS variant k (initial state only: never solved)"""
    t = w.twin()
    if BIG_BIAS[k % 4] is not None:
        t.speed_bias[t.F - 1, 3:6], t.speed_bias[t.F - 1, 6:9] = BIG_BIAS[k % 4]
    return t


def failure_windows(group, state):
    """the windows of a failure-detection parity batch: at the initial state two twins per shape with biases of variants 0 .. 3 in turn"""
    if state in ("solved", "solved alt"):
        return [solved_window(n, state == "solved alt").twin() for n in group if n in SOLVED]
    return [with_big_bias(shape_window(n), 2 * i + j) for i, n in enumerate(group) for j in range(2)]


def failure_cases():
    """(tag, pose_n, sb_n, tracks, last_pose [7]) of every case of the GPU parity test"""
    out = []
    for gname, group in (("leg", LEG_GROUP), ("imu", IMU_GROUP)):
        for state in ("initial", "solved", "solved alt"):
            ws = failure_windows(group, state)
            for shift in (0, 1, 2, 3):
                tracks, last = failure_inputs(ws, shift)
                for i, w in enumerate(ws):
                    out.append(("%s %s window %d shift %d" % (gname, state, i, shift), w.pose[w.F - 1].copy(), w.speed_bias[w.F - 1].copy(), int(tracks[i]), last[i]))
    return out


# ---- option checks -----------------------------------------------------------------------------------------------------------------
def test_option_checks_need_no_device():
    from cerberus_amd import api, _ctypes as T
    o, a = api.gauge_opts()
    assert (o.anchor, o.reserved, a) == (T.GAUGE_ANCHOR["uploaded"], 0, None)
    o, a = api.gauge_opts("given", np.zeros((3, 7)), 3)
    assert o.anchor == T.GAUGE_ANCHOR["given"] and a.shape == (3, 7) and a.flags["C_CONTIGUOUS"]
    with pytest.raises(ValueError, match="needs anchor_pose"):
        api.gauge_opts("given")
    with pytest.raises(ValueError, match="needs anchor='given'"):
        api.gauge_opts("uploaded", np.zeros((1, 7)))
    with pytest.raises(ValueError, match="anchor must be one of"):
        api.gauge_opts("frame0")
    for bad in (np.zeros((3, 6)), np.zeros((2, 7)), np.zeros(21), np.zeros((3, 7, 1))):
        with pytest.raises(ValueError, match="shape"):
            api.gauge_opts("given", bad, 3)
    t, p = api.failure_inputs(2, [1, 2], np.zeros((2, 7)))
    assert t.dtype == np.int32 and p.shape == (2, 7)
    assert api.failure_inputs(2) == (None, None)
    for kw in (dict(last_track_num=[1, 2, 3]), dict(last_pose=np.zeros((2, 6))), dict(last_pose=np.zeros((3, 7))), dict(last_track_num=np.zeros((2, 1)))):
        with pytest.raises(ValueError, match="shape"):
            api.failure_inputs(2, **kw)
    assert C_sizes() == (8, 16, 12)


def C_sizes():
    import ctypes as C
    from cerberus_amd import _ctypes as T
    return C.sizeof(T.GaugeOpts), C.sizeof(T.WindowGaugeRecord), C.sizeof(T.WindowFailureRecord)


# ---- the definition against the oracle -----------------------------------------------------------------------------------------------
def _oracle_fix(anchor, pose, sb, ex, w):
    """the oracle's gauge fix (all 11 frames, as the reference's) of a state given as arrays; w lends the other arrays"""
    from oracle import oracle_py as O
    t = w.twin()
    before = t.clone_state()
    before[0][0] = anchor
    t.pose[...], t.speed_bias[...], t.ex_pose[...] = pose, sb, ex
    O.gauge_fix(before, t)
    return t.pose.copy(), t.speed_bias.copy(), t.ex_pose.copy()


def test_definition_matches_the_oracle_on_the_golden_cases():
    """the 13 Euler-singularity cases: against the oracle's gauge fix and against the fixture's recorded result of the reference's own
    arithmetic, at the tolerance tests/test_golden.py uses for this golden (1e-12 absolute); the singular flag is the fixture's"""
    worst = 0.0
    for n, (w, a) in enumerate(golden_windows()):
        r = G.window_gauge_fix(w, a)
        assert r.status == G.GAUGE_OK and r.singular == int(GG["branch_taken"][n]), n
        op, os_, oe = _oracle_fix(a, w.pose, w.speed_bias, w.ex_pose, w)
        for got, orc, gold in ((r.pose, op, GG["fixed_pose_%d" % n]), (r.speed_bias, os_, GG["fixed_sb_%d" % n]), (r.ex_pose, oe, GG["fixed_ex_%d" % n])):
            worst = max(worst, np.abs(got - orc).max(), np.abs(got - gold).max())
            np.testing.assert_allclose(got, orc, rtol=0, atol=1e-12, err_msg="case %d against the oracle" % n)
            np.testing.assert_allclose(got, gold, rtol=0, atol=1e-12, err_msg="case %d against the fixture" % n)
    print("MEASURED gauge_ref against the oracle and the golden, 13 cases: %.1e (bound 1e-12)" % worst)


def test_definition_matches_the_oracle_on_random_windows():
    rng = np.random.default_rng(11)
    w = shape_window("F11")
    worst = 0.0
    for _ in range(20):
        pose, sb, ex = rng.normal(size=(11, 7)), rng.normal(size=(11, 9)), rng.normal(size=(2, 7))
        pose[:, :3] *= 3
        anchor = rng.normal(size=7)
        anchor[3:] /= np.linalg.norm(anchor[3:])   # (Rs[0] is a rotation in the reference; the solved quaternions need not be unit)
        pose[0, 3:] /= np.linalg.norm(pose[0, 3:])
        r = G.gauge_fix(anchor, pose, sb, ex)
        op, os_, oe = _oracle_fix(anchor, pose, sb, ex, w)
        e = max(G.gauge_error((r.pose, r.speed_bias, r.ex_pose), (op, os_, oe), 11), np.abs(r.speed_bias[:, 3:] - sb[:, 3:]).max())
        worst = max(worst, e)
        assert e <= 1e-12
    print("MEASURED gauge_ref against the oracle, 20 random windows: %.1e (bound 1e-12)" % worst)


def test_constant_extrinsics_cases_can_tell_a_rewrite():
    """F11ex and F11exfree are one window whose extrinsic quaternions the normalised rewrite moves: at the initial and at the solved
    state the definition leaves the constant block as uploaded where a rewrite would move both its rows, rewrites the free twin's, and
    does not read a constant block (a NaN there is no NUMERIC). The synthetic quaternion of the other shapes comes back with the
    same bits."""
    plain = shape_window("F11")
    assert G.window_gauge_fix(plain, plain.pose[0]).ex_pose.tobytes() == plain.ex_pose.tobytes()
    for get in (shape_window, solved_window):
        const, free = get("F11ex"), get("F11exfree")
        assert const.ex_const and not free.ex_const
        assert shape_window("F11ex").ex_pose.tobytes() == shape_window("F11exfree").ex_pose.tobytes() == const.ex_pose.tobytes()
        a = given_anchor(shape_window("F11ex").pose[0], 1)
        # rf: the constant window's state fixed as if its extrinsics were free: what a kernel that ignored ex_const would write (the
        # solver has normalised the free twin's quaternions itself by the time it is solved, so that twin shows it at the initial state)
        rc, rf = G.window_gauge_fix(const, a), G.gauge_fix(a, const.pose, const.speed_bias, const.ex_pose, False)
        assert rc.status == rf.status == G.GAUGE_OK
        assert rc.ex_pose.tobytes() == const.ex_pose.tobytes() == shape_window("F11ex").ex_pose.tobytes()
        if get is shape_window:
            assert G.window_gauge_fix(free, a).ex_pose.tobytes() == rf.ex_pose.tobytes()
        for k in range(2):
            assert rf.ex_pose[k, :3].tobytes() == const.ex_pose[k, :3].tobytes()
            # (Quaterniond(Matrix3d) may return -q: the turned quaternion's w is near -0.5, the matrix's trace near 0)
            moved = min(np.abs(rf.ex_pose[k, 3:] - const.ex_pose[k, 3:]).max(), np.abs(rf.ex_pose[k, 3:] + const.ex_pose[k, 3:]).max())
            assert 1e-10 < moved < 1e-8, (k, moved)   # the 3e-9 / 2e-9 the quaternion is off unit length: far above a rounding
        bad_c, bad_f = const.twin(), free.twin()
        bad_c.ex_pose[1, 5] = bad_f.ex_pose[1, 5] = np.nan
        assert G.window_gauge_fix(bad_c, a).status == G.GAUGE_OK and G.window_gauge_fix(bad_f, a).status == G.GAUGE_NUMERIC
        assert G.window_gauge_fix(bad_c, a).pose.tobytes() == rc.pose.tobytes()


# ---- floors ------------------------------------------------------------------------------------------------------------------------
def _moved(a, rng):
    a = np.asarray(a, float)
    return np.nextafter(a, np.where(rng.random(a.shape) < 0.5, -np.inf, np.inf))


def test_fp64_floor_measured():
    """DESIGN §4.13's rule over every case of the GPU parity test: (a) every input moved one unit in the last place, (b) the same formulas
    in numpy.longdouble. gauge_ref.FLOOR / FLOOR_FAILURE are the measured values rounded up."""
    rng = np.random.default_rng(5)
    ld = np.longdouble
    fa = fb = ya = yb = 0.0
    for tag, anchor, pose, sb, ex, exc in gauge_cases():
        r = G.gauge_fix(anchor, pose, sb, ex, exc)
        rl = G.gauge_fix(anchor, pose, sb, ex, exc, dtype=ld)
        assert r.status == rl.status == G.GAUGE_OK and r.singular == rl.singular, tag
        F = len(pose)
        b = G.gauge_error((r.pose, r.speed_bias, r.ex_pose), (rl.pose, rl.speed_bias, rl.ex_pose), F)
        a = 0.0
        for _ in range(4):
            rm = G.gauge_fix(_moved(anchor, rng), _moved(pose, rng), _moved(sb, rng), _moved(ex, rng), exc)
            assert rm.singular == r.singular, tag
            a = max(a, G.gauge_error((rm.pose, rm.speed_bias, rm.ex_pose), (r.pose, r.speed_bias, r.ex_pose), F))
            if not r.singular:
                ya = max(ya, abs(rm.yaw_diff_deg - r.yaw_diff_deg) / 180)
        if not r.singular:
            yb = max(yb, abs(rl.yaw_diff_deg - r.yaw_diff_deg) / 180)
        fa, fb = max(fa, a), max(fb, b)
    print("MEASURED gauge fix floor: (a) one ulp %.1e, (b) longdouble %.1e; yaw_diff_deg / 180: (a) %.1e (b) %.1e; FLOOR %.0e, TOL %.0e" % (fa, fb, ya, yb, G.FLOOR, G.TOL))
    assert max(fa, fb, ya, yb) <= G.FLOOR and G.TOL == 10 * G.FLOOR
    assert G.FLOOR <= 4 * max(fa, fb, ya, yb), "FLOOR is the measured value rounded up, not a loose bound"
    va = vb = 0.0
    for tag, pn, sn, tr, lp in failure_cases():
        r = G.failure_detection(pn, sn, tr, lp)
        rl = G.failure_detection(pn, sn, tr, lp, dtype=ld)
        assert r.flags == rl.flags and r.status == G.FAILURE_OK, tag
        vb = max(vb, G.values_error(r.values, rl.values))
        for _ in range(4):
            rm = G.failure_detection(_moved(pn, rng), _moved(sn, rng), tr, _moved(lp, rng))
            assert rm.flags == r.flags, tag
            va = max(va, G.values_error(rm.values, r.values))
    print("MEASURED failure detection floor: (a) one ulp %.1e, (b) longdouble %.1e; FLOOR_FAILURE %.0e, TOL_FAILURE %.0e" % (va, vb, G.FLOOR_FAILURE, G.TOL_FAILURE))
    assert max(va, vb) <= G.FLOOR_FAILURE and G.TOL_FAILURE == 10 * G.FLOOR_FAILURE
    assert G.FLOOR_FAILURE <= 4 * max(va, vb), "FLOOR_FAILURE is the measured value rounded up, not a loose bound"


# ---- discrimination ----------------------------------------------------------------------------------------------------------------
def test_parity_inputs_tell_the_definition_from_its_plausible_mistakes():
    """every gauge-fix parity case moves by 1e6 TOL or more when the velocities are not rotated and when the solved frame 0 is taken for
    the anchor; every failure-detection case when pi stands for 3.14 and when Ba and Bg are swapped; and at least one case changes a
    flag bit under each of the latter two"""
    least = {}
    for tag, anchor, pose, sb, ex, exc in gauge_cases():
        r = G.gauge_fix(anchor, pose, sb, ex, exc)
        for wrong in ("no_velocity_rotation", "anchor_solved"):
            m = G.gauge_fix(anchor, pose, sb, ex, exc, wrong=wrong)
            e = G.gauge_error((m.pose, m.speed_bias, m.ex_pose), (r.pose, r.speed_bias, r.ex_pose), len(pose))
            least[wrong] = min(least.get(wrong, np.inf), e)
            assert e >= 1e6 * G.TOL, (tag, wrong, e)
    flips = {"pi": 0, "swap_biases": 0}
    for tag, pn, sn, tr, lp in failure_cases():
        r = G.failure_detection(pn, sn, tr, lp)
        for wrong in flips:
            m = G.failure_detection(pn, sn, tr, lp, wrong=wrong)
            e = G.values_error(m.values, r.values)
            least[wrong] = min(least.get(wrong, np.inf), e)
            assert e >= 1e6 * G.TOL_FAILURE, (tag, wrong, e)
            flips[wrong] += int(m.flags != r.flags)
    print("MEASURED least effect of each mistake over the parity cases: %s (1e6 TOL = %.0e, 1e6 TOL_FAILURE = %.0e); flag flips %s"
          % ({k: "%.1e" % v for k, v in least.items()}, 1e6 * G.TOL, 1e6 * G.TOL_FAILURE, flips))
    assert all(flips.values())


def test_no_failure_criterion_near_its_threshold():
    """every compared quantity of every parity case is 1e-6 relative or more away from its threshold (no flag can flip by rounding), every
    flag bit is set on some case and clear on another, and no gauge-fix case has a pitch within 1e-3 degrees of the branch's edge"""
    seen_set, seen_clear = 0, 0
    for tag, pn, sn, tr, lp in failure_cases():
        r = G.failure_detection(pn, sn, tr, lp)
        for v, t in list(zip(r.values, G.THRESHOLDS))[1:]:   # (the track count is an integer: its comparison does not round)
            assert abs(v - t) >= 1e-6 * t, (tag, v, t)
        seen_set |= r.flags
        seen_clear |= ~r.flags & 63
        assert r.would_reboot == int(bool(r.flags & 6))
    assert seen_set == 63 and seen_clear == 63
    singular = 0
    for tag, anchor, pose, sb, ex, exc in gauge_cases():
        from deadreckon_ref import quat_R
        for q in (anchor[3:7], pose[0, 3:7]):
            p = abs(G.R2ypr_deg(quat_R(q))[1])
            assert abs(abs(p - 90) - 1.0) >= 1e-3, (tag, p)
        singular += G.gauge_fix(anchor, pose, sb, ex, exc).singular
    assert 8 <= singular < len(gauge_cases()) - 8
