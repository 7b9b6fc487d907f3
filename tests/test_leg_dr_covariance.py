"""CPU: the numpy definition of vilo_batch_leg_dead_reckon_covariance (tests/leg_dr_cov_ref.py, written from the reference's lines): the
measured FP64 floor that sets the tolerance (leg_dr_cov_ref.TOL = 10 x FLOOR), its tie to the pinned preintegration
record T (Phi Sigma_0' Phi^T + Sigma_rec) T^T, the mistakes that must show, the branches its inputs reach, the statuses, the CPU path of
cerberus_amd/csrc/legdrcov_host.hpp (the block builders and products the kernel calls) against the definition in a stand-alone program
built with the address and undefined-behaviour sanitizers (tests/host_check/leg_dr_cov_check.cpp, run as a child process; nothing is loaded
into Python), the wrapper's options, the struct sizes and the library's exports. tests/test_leg_dr_covariance_gpu.py takes its cases from here."""
import ctypes as C
import functools
import os
import subprocess

import numpy as np
import pytest

import leg_dr_cov_ref as R
import leg_dr_model as L
from conftest import ROOT
from test_dead_reckon import frames_window, take
from test_gyro_align import kind_window
from test_leg_dead_reckon import EXPLICIT, MODELS, _header_struct, branch_cases, cases as nominal_cases, model_cfg, tie_inputs


@functools.lru_cache(maxsize=None)
def cov_cfg(model):
    """the configuration of a contact model: test_leg_dead_reckon's, and under model 1 (whose arithmetic is model 0's) a dphi_n that is
    not phi_n, which the default configuration has equal: a swap of the two must show somewhere"""
    import copy
    c = copy.copy(model_cfg(model))
    if model == 1:
        c.dphi_n = 3.0 * c.phi_n
    return c


def spd19(seed, scale=1e-4):
    """a 19 x 19 covariance of the size a solved window's frame block has, with every cross term present"""
    g = np.random.default_rng(seed)
    A = g.normal(size=(19, 19))
    d = scale * np.array([1.0] * 3 + [0.1] * 3 + [1.0] * 3 + [0.3] * 3 + [0.03] * 3 + [0.1] * 4)
    return (A @ A.T / 19 + np.eye(19)) * np.outer(d, d)


@functools.lru_cache(maxsize=None)
def cases():
    """(tag, model, window, samples [n, 35], from_frame, cov_in or None): the nominal call's cases (ranges of 0, 1, 2, 3 and 12 samples,
    from_frame -1 and 4, windows of 2 and 11 frames, the three contact models, the three branch inputs), each with cov_in None and, for
    the stepping ones with from_frame -1 and the 2-frame windows, with a given cov_in"""
    out = []
    for i, (tag, m, w, s, f) in enumerate(nominal_cases()):
        out.append((tag + ", cov_in None", m, w, s, f, None))
        if f != EXPLICIT:
            out.append((tag + ", cov_in given", m, w, s, f, spd19(i)))
    return tuple(out)


def is_all_air(case):
    return case[0].startswith("all feet in the air")


@functools.lru_cache(maxsize=None)
def _ref(i, dtype_name="float64"):
    tag, m, w, s, f, ci = cases()[i]
    return R.window_leg_dr_cov(cov_cfg(m), w, s, f, ci, dtype=getattr(np, dtype_name))


def reference(i):
    return _ref(i)


def parts(r):
    return (r.cov, r.pose_cov_trajectory, r.leg_cov_trajectory)


def _ulp_moved(case, seed):
    tag, m, w, s, f, ci = case
    g = np.random.default_rng(seed)
    mv = lambda a: np.nextafter(a, a + np.where(g.random(a.shape) < 0.5, -1.0, 1.0) * np.maximum(np.abs(a), 1e-300))   # noqa: E731
    w2 = w.twin()
    w2.pose[...] = mv(w.pose); w2.speed_bias[...] = mv(w.speed_bias); w2.leg_bias[...] = mv(w.leg_bias)
    s2 = mv(np.asarray(s, float))
    s2[:, 31:35] = np.asarray(s, float).reshape(-1, 35)[:, 31:35] if m != 2 else s2[:, 31:35]   # (contact flags are 0 / 1: not moved)
    return (tag, m, w2, s2, f, None if ci is None else mv(ci))


def test_fp64_floor_measured():
    """The floor as section 4.29 measures it: the definition in float64 against numpy.longdouble, and every input moved one unit in the
    last place, over the cases; the all-feet-in-the-air case in a group of its own. FLOOR covers the largest and is no loose cover."""
    assert np.finfo(np.longdouble).eps < 1e-18
    worst = {"precision": 0.0, "ulp": 0.0, "air precision": 0.0, "air ulp": 0.0}
    for i, case in enumerate(cases()):
        r = reference(i)
        assert r.status == L.OK, case[0]
        if r.n_steps == 0:
            continue
        x = _ref(i, "longdouble")
        k = "air " if is_all_air(case) else ""
        worst[k + "precision"] = max(worst[k + "precision"], R.cov_error(parts(r), parts(x)))
        tag, m, w2, s2, f, ci2 = _ulp_moved(case, i)
        y = R.window_leg_dr_cov(cov_cfg(m), w2, s2, f, ci2, dtype=np.longdouble)
        if L.flags_of((y.state, y.legs, np.zeros((0, L.TRAJ)))).tobytes() == L.flags_of((x.state, x.legs, np.zeros((0, L.TRAJ)))).tobytes():
            worst[k + "ulp"] = max(worst[k + "ulp"], R.cov_error(parts(y), parts(x)))
    print("MEASURED floor: %s (FLOOR %.0e, TOL %.0e)" % (", ".join("%s %.2e" % kv for kv in sorted(worst.items())), R.FLOOR, R.TOL))
    top = max(worst.values())
    assert top <= R.FLOOR
    assert top >= 0.1 * R.FLOOR   # (the constant is what is measured, not a loose cover)
    assert R.TOL == 10 * R.FLOOR


def test_no_step_is_sigma0_bit_for_bit():
    for i, case in enumerate(cases()):
        r = reference(i)
        if r.n_steps == 0:
            want = R.sym(R.embed(case[5], np.float64))
            assert r.cov.tobytes() == want.tobytes(), case[0]
            if case[5] is not None:
                assert want[9:12, 9:12].tobytes() == np.ascontiguousarray(want[0:3, 0:3]).tobytes() and want[9:12, 3:6].tobytes() == np.ascontiguousarray(want[0:3, 3:6]).tobytes()


@functools.lru_cache(maxsize=None)
def solved_blocks():
    """tests/golden/leg_dr_cov_solved_blocks.npz: the 19 x 19 frame blocks Batch.covariance(gauge="frame0") gives after a 4-iteration solve
    of tests/test_covariance_gpu.py's windows of seeds 11 and 12 (60 landmarks), cut by api.leg_dr_cov_in at from_frame -1 and 3: [4, 19, 19].
    tests/test_leg_dr_covariance_gpu.py makes them again on the device and holds the file to them."""
    return np.load(os.path.join(ROOT, "tests", "golden", "leg_dr_cov_solved_blocks.npz"))["blocks"]


def _tie_gap(cfg, ocfg, s, lin, R_f, S0, rec_of):
    steps, _ = R.propagate(cfg, lin, s, R_f, S0)
    xl, _ = R.propagate(cfg, lin, s, R_f, S0, np.longdouble)
    want = R.from_record(rec_of(), R_f, S0)
    ref = xl[-1].astype(np.float64)
    return R._rel(steps[-1], want), R._rel(steps[-1], ref), R._rel(want, ref)


def test_tie_to_the_pinned_record():
    """The definition against T (Phi Sigma_0' Phi^T + Sigma_rec) T^T of the oracle's record (tests/test_oracle_vs_reference.py pins it)
    and of the reference's own records (tests/golden/preint_contact_edges.npz), at cov_in None, at a solved window's frame block
    (solved_blocks(), one of the four per interval in turn) and at a synthetic one, R_f the identity and a real rotation, under the three
    contact models. Both sides chain the same normalised delta_q, so the gap is rounding: it is measured
    with the long-double definition as the yardstick and gated at ten times that floor."""
    from oracle import oracle_py as O
    import deadreckon_ref as D
    R_f = D.quat_R(D.quat_normalized(np.array([0.3, -0.2, 0.5, 0.78]), np.float64), np.float64)
    worst = dict(gap=0.0, mine=0.0, record=0.0)
    for n, (tag, m, s, lin, gold) in enumerate(tie_inputs()):
        cfg = cov_cfg(m)
        ocfg = O.config_from(cfg)
        rec = O.preintegrate_imu_leg(ocfg, s, lin)
        for Rf in (np.eye(3), R_f):
            for S0 in (np.zeros((31, 31)), R.embed(solved_blocks()[n % 4], np.float64), R.embed(spd19(3), np.float64)):
                for which, r in (("oracle", rec), ("reference", gold)):
                    if r is None:
                        continue
                    gap, mine, record = _tie_gap(cfg, ocfg, s, lin, Rf, S0, lambda: r)
                    worst["gap"], worst["mine"], worst["record"] = max(worst["gap"], gap), max(worst["mine"], mine), max(worst["record"], record)
                    assert gap <= R.TOL, (tag, which, gap)
    print("MEASURED tie: definition to record formula %.2e; to the long-double definition: definition %.2e, record formula %.2e (gate %.0e)" %
          (worst["gap"], worst["mine"], worst["record"], R.TOL))


MISTAKE_CASE = {
    "no_vqv": "model 0, 3 samples, from_frame -1, cov_in None",
    "f_transposed": "model 0, 12 samples, from_frame -1, cov_in given",
    "pre_rotation": "model 0, 12 samples, from_frame -1, cov_in None",
    "acc_n_for_z": "model 0, 12 samples, from_frame -1, cov_in None",
    "q_flag_independent": "flag of leg 1 crosses mid-range, model 0, cov_in None",
    "no_override": "all feet in the air, cov_in None",
    "phi_dphi_swapped": "model 1, 12 samples, from_frame -1, cov_in None",
    "no_rho_column": "model 0, 12 samples, from_frame -1, cov_in None",
    "unc_squared": "model 0, 12 samples, from_frame -1, cov_in None",
    "no_dp_eps": "model 0, 3 samples, from_frame -1, cov_in given",
}


@pytest.mark.parametrize("wrong", R.MISTAKES)
def test_each_mistake_shows(wrong):
    """the definition with one thing wrong moves the answer by at least 1000 x TOL on the named case"""
    idx = [i for i, c in enumerate(cases()) if c[0] == MISTAKE_CASE[wrong]]
    assert len(idx) == 1, MISTAKE_CASE[wrong]
    tag, m, w, s, f, ci = cases()[idx[0]]
    good = reference(idx[0])
    bad = R.window_leg_dr_cov(cov_cfg(m), w, s, f, ci, wrong=wrong)
    e = R.cov_error(parts(bad), parts(good))
    print("MEASURED %s on '%s': %.2e (needs %.0e)" % (wrong, tag, e, 1000 * R.TOL))
    assert e >= 1000 * R.TOL


def test_branch_inputs_sit_where_claimed():
    for tag, m, w, s, f, what in branch_cases():
        r = R.window_leg_dr_cov(cov_cfg(m), w, s, f)
        assert r.status == L.OK and r.n_steps == 11, tag
        if what == "all_air":
            assert r.branches["all_air"] == r.n_steps and not r.branches["flags"].any(), tag
            dt = np.asarray(s).reshape(-1, 35)[1:, 0]
            # the override decides the answer: every leg's position variance is the sum of 10e10 dt^2 to first order
            assert np.allclose(np.diagonal(r.leg_cov_trajectory[-1], axis1=-2, axis2=-1), 10e10 * (dt * dt).sum(), rtol=1e-6), tag
        elif what == "clamped":
            assert r.branches["clamped"] > 0, tag
        else:
            fl = r.branches["flags"][:, 1]
            assert fl[0] == 1.0 and fl[-1] == 0.0 and set(fl) == {0.0, 1.0}, (tag, fl)
            # the lifted foot's variance grows by v_n_max dt^2 a step after the crossing, the standing feet's by v_n_min
            d = np.diff(r.leg_cov_trajectory[:, :, 0, 0], axis=0)
            assert d[-1, 1] > 100 * d[-1, 0] and (m == 2 or d[0, 1] < 10 * d[0, 0]), tag


def test_statuses_of_the_definition():
    w, two = kind_window("L9", 1), frames_window(2)
    cfg = cov_cfg(0)
    s = take(w, 12, 0)
    r = R.window_leg_dr_cov(cfg, two, s, 5)
    assert r.status == L.NO_FRAME and r.n_steps == 11 and not r.cov.any() and not r.pose_cov_trajectory.any() and not r.leg_cov_trajectory.any()
    ci = spd19(1)
    bad = ci.copy()
    bad[2, 7] = np.nan
    r = R.window_leg_dr_cov(cfg, w, s, -1, bad)
    assert r.status == L.NUMERIC and not r.cov.any() and not r.state.any()
    low = ci.copy()
    low[7, 2] = np.nan   # below the diagonal: not read
    a, b = R.window_leg_dr_cov(cfg, w, s, -1, low), R.window_leg_dr_cov(cfg, w, s, -1, ci)
    assert a.status == L.OK and a.cov.tobytes() == b.cov.tobytes()
    sn = s.copy()
    sn[7, 25] = np.nan
    assert R.window_leg_dr_cov(cfg, w, sn).status == L.NUMERIC


# ------------------------------------------------------------------------------ the CPU path of legdrcov_host.hpp, in a sanitized program
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("leg_dr_cov") / "leg_dr_cov_check")
    src = os.path.join(ROOT, "tests", "host_check", "leg_dr_cov_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                   check=True, timeout=300)
    return exe


def run_host(exe, tmp, cfg, items):
    """items: (pose [7], speed_bias [9], leg_bias [4], cov_in or None, samples [n, 35]) per window. Returns per window
    (status, n_steps, state, legs, cov, pose_traj, leg_traj)."""
    cfg_d = np.frombuffer(bytes(cfg), dtype=np.float64)
    parts_ = [np.array([float(len(items))]), cfg_d]
    for pose, sb, lb, ci, s in items:
        s = np.asarray(s, np.float64).reshape(-1, 35)
        parts_ += [np.array([float(len(s)), 0.0 if ci is None else 1.0]), np.asarray(pose, np.float64), np.asarray(sb, np.float64), np.asarray(lb, np.float64)]
        if ci is not None:
            parts_.append(np.asarray(ci, np.float64).ravel())
        parts_.append(s.ravel())
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    np.concatenate(parts_).tofile(fin)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.returncode, p.stdout, p.stderr)
    o = np.fromfile(fout, dtype=np.float64)
    out, at = [], 0
    for _ in items:
        status, n_steps = int(o[at]), int(o[at + 1])
        at += 2
        state, legs, cov = o[at:at + 32], o[at + 32:at + 44].reshape(4, 3), o[at + 44:at + 44 + 961].reshape(31, 31)
        at += 44 + 961
        pt = o[at:at + 36 * n_steps].reshape(n_steps, 6, 6)
        lt = o[at + 36 * n_steps:at + 72 * n_steps].reshape(n_steps, 4, 3, 3)
        at += 72 * n_steps
        out.append((status, n_steps, state, legs, cov, pt, lt))
    assert at == len(o)
    return out


def test_host_program_self_checks_under_sanitizers(host_program):
    p = subprocess.run([host_program], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip() == "ok", p.stdout


def test_host_path_matches_the_definition(host_program, tmp_path):
    """The CPU recurrence, under the sanitizers, on every case: within the tolerance of the definition, no-step cases bit for bit; the
    nominal rows, the last trajectory rows and the call without trajectories are checked bit for bit by the program itself"""
    worst = 0.0
    for m in MODELS:
        mine = [(i, c) for i, c in enumerate(cases()) if c[1] == m]
        items = []
        for i, (tag, _, w, s, f, ci) in mine:
            f = w.F - 1 if f == -1 else f
            items.append((w.pose[f], w.speed_bias[f], w.leg_bias[f], ci, s))
        for (i, case), (status, n_steps, state, legs, cov, pt, lt) in zip(mine, run_host(host_program, str(tmp_path), cov_cfg(m), items)):
            ref = reference(i)
            assert (status, n_steps) == (ref.status, ref.n_steps), case[0]
            assert cov.tobytes() == cov.T.copy().tobytes(), case[0]
            if n_steps == 0:
                assert cov.tobytes() == ref.cov.tobytes(), case[0]
                continue
            e = R.cov_error((cov, pt, lt), parts(ref))
            worst = max(worst, e)
            assert e <= R.TOL, (case[0], e)
    print("MEASURED host program against the definition: %.2e (tolerance %.0e)" % (worst, R.TOL))


def test_host_path_statuses(host_program, tmp_path):
    w = kind_window("L9", 1)
    f = w.F - 1
    s = take(w, 12, 0)
    sn = s.copy()
    sn[7, 25] = np.nan
    ci = spd19(2)
    bad, low = ci.copy(), ci.copy()
    bad[2, 7] = np.nan
    low[7, 2] = np.nan
    base = (w.pose[f], w.speed_bias[f], w.leg_bias[f])
    res = run_host(host_program, str(tmp_path), cov_cfg(0), [base + (ci, s), base + (None, sn), base + (bad, s), base + (low, s)])
    assert [r[0] for r in res] == [L.OK, L.NUMERIC, L.NUMERIC, L.OK]
    for r in res[1:3]:
        assert not any(a.any() for a in r[2:])
    for a, b in zip(res[0][2:], res[3][2:]):
        assert a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------ the wrapper and the header
def test_wrapper_options_and_cov_in_need_no_device():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    o = api.leg_dr_cov_opts()
    assert (o.from_frame, o.reserved) == (-1, 0) and api.leg_dr_cov_opts(3).from_frame == 3
    for bad in (-2, T.MAX_FRAMES, 1.5):
        with pytest.raises(ValueError):
            api.leg_dr_cov_opts(bad)
    assert api.LegDeadReckonedCovariance._fields == ("state", "legs", "cov", "pose_cov_trajectory", "leg_cov_trajectory", "step_offsets", "n_steps", "status")
    assert (T.LEG_DR_COV_N, T.LEG_DR_COV_IN, T.LEG_DR_COV_POSE) == (R.N, R.N_IN, 6) and T.LEG_DR_COV_IN == T.COV_FRAME
    assert hasattr(api.Batch, "leg_dead_reckon_covariance") and hasattr(api.Context, "window_leg_dead_reckon_covariance")
    frames = np.random.default_rng(0).normal(size=(3, T.F, 19, 19))
    n_frames = np.array([11, 2, 5])
    a = api.leg_dr_cov_in(frames, n_frames)
    assert a.shape == (3, 19, 19) and a[0].tobytes() == frames[0, 10].tobytes() and a[1].tobytes() == frames[1, 1].tobytes() and a[2].tobytes() == frames[2, 4].tobytes()
    b = api.leg_dr_cov_in(frames, n_frames, 4)
    assert b[0].tobytes() == frames[0, 4].tobytes() and not b[1].any() and b[2].tobytes() == frames[2, 4].tobytes()
    with pytest.raises(ValueError):
        api.leg_dr_cov_in(frames[:, :, :15, :15], n_frames)
    with pytest.raises(ValueError):
        api.leg_dr_cov_in(frames, n_frames[:2])


def test_struct_sizes_match_the_header():
    from cerberus_amd import _ctypes as T
    fields = _header_struct("vilo_leg_dr_cov_opts")
    assert [f for f, _ in T.LegDrCovOpts._fields_] == [f[-1] for f in fields] and all(f[0] == "int32_t" for f in fields)
    assert C.sizeof(T.LegDrCovOpts) == 4 * len(fields) == 8
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    assert "cov_out[w][31][31]" in hdr and "cov_in[w][19][19]" in hdr and "[sum n_steps][4][3][3]" in hdr


def test_library_exports_the_entry_points():
    from cerberus_amd import _ctypes as T
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for name in ("vilo_default_leg_dr_cov_opts", "vilo_batch_leg_dead_reckon_covariance", "vilo_window_leg_dead_reckon_covariance", "vilo_last_leg_dr_cov_ms"):
        assert hasattr(lib, name), name
    o = T.LegDrCovOpts(7, 7)
    lib.vilo_default_leg_dr_cov_opts(C.byref(o))   # host code: needs no device
    assert (o.from_frame, o.reserved) == (-1, 0)
