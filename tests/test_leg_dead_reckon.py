"""CPU: the numpy definition of vilo_batch_leg_dead_reckon (tests/leg_dr_model.py, written from the reference's lines): the measured FP64
floor that sets the tolerance (leg_dr_model.TOL = 10 x leg_dr_model.FLOOR), the branches its inputs reach, the tie of
delta_q / delta_v / delta_eps to the oracle's preintegration record and to the reference's own records of
tests/golden/preint_contact_edges.npz under all three contact models, the CPU path of cerberus_amd/csrc/legdr_host.hpp (legdr_step, the
function the kernel calls) against the definition, in a stand-alone program built with the address and undefined-behaviour sanitizers
(tests/host_check/leg_dr_check.cpp, run as a child process; nothing is loaded into Python), the statuses, the wrapper's options, the
struct sizes and the library's exports. tests/test_leg_dead_reckon_gpu.py takes its cases from here.

sum_delta_eps, the weights and the flags have no public counterpart in the pinned oracle: for them the definition is the only reference
("restated, unpinned")."""
import copy
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import leg_dr_model as L
from conftest import ROOT
from test_dead_reckon import frames_window, take
from test_gyro_align import kind_window

RANGES = (0, 1, 2, 3, 12)   # samples of a range: no step twice over, one, two, and eleven steps: the five-slot force window wraps twice
MODELS = (0, 1, 2)          # contact_sensor_type
EXPLICIT = 4                # the explicit from_frame of the 11-frame windows


@functools.lru_cache(maxsize=None)
def model_cfg(model):
    from cerberus_amd import synth
    c = copy.copy(synth.default_config())
    c.contact_sensor_type = model
    return c


def forces(samples, seed):
    """the samples with their contact columns turned into foot forces for contact_sensor_type 2: 15 N + 140 N on a standing foot + noise"""
    s = np.array(samples, dtype=np.float64, copy=True).reshape(-1, 35)
    s[:, 31:35] = 15.0 + 140.0 * s[:, 31:35] + 4.0 * np.random.default_rng(seed).normal(size=(len(s), 4))
    return s


def for_model(samples, model, seed=0):
    return forces(samples, 100 + seed) if model == 2 else np.array(samples, dtype=np.float64, copy=True).reshape(-1, 35)


def in_the_air(samples):
    """all four feet off the ground for the whole range (contact models 0 / 1): imu_leg_integration_base.cpp:354-358"""
    s = np.array(samples, copy=True)
    s[:, 31:35] = 0.0
    return s


def clamping(samples):
    """contact model 2 with one leg's joint velocities a million times the gait's: (lo_v - delta_v)^2 takes that leg's weights under 0.001"""
    s = forces(samples, 7)
    s[:, 19 + 3:19 + 6] *= 1e6
    return s


def crossing(samples, model):
    """leg 1 stands for the first half of the range and is lifted for the second: its flag crosses 0.5 mid-range"""
    s = np.array(samples, copy=True)
    h = len(s) // 2
    s[:h, 32], s[h:, 32] = 1.0, 0.0
    return forces(s, 9) if model == 2 else s


def branch_cases():
    """(tag, model, window, samples, from_frame, what the definition must report) of the three branch inputs"""
    w = kind_window("L9", 1)
    base = take(w, 12, 20)
    out = [("all feet in the air", 0, w, in_the_air(base), -1, "all_air"),
           ("a weight at the 0.001 clamp", 2, w, clamping(base), -1, "clamped")]
    for m in MODELS:
        out.append(("flag of leg 1 crosses mid-range, model %d" % m, m, w, crossing(base, m), EXPLICIT, "crossing"))
    return out


def cases():
    """(tag, model, window, samples [n, 35], from_frame) of every case the host program and the GPU parity test compare"""
    out = []
    w, two = kind_window("L9", 1), frames_window(2)
    for m in MODELS:
        for i, n in enumerate(RANGES):
            for f in (-1, EXPLICIT):
                out.append(("model %d, %d samples, from_frame %d" % (m, n, f), m, w, for_model(take(w, n, 5 * i + 2), m, i), f))
        out.append(("model %d, 2-frame window, 12 samples, from_frame 0" % m, m, two, for_model(take(two, 12, 3), m, 5), 0))
    out += [c[:5] for c in branch_cases()]
    return out


def reference(case):
    tag, m, w, s, f = case
    r = L.window_leg_dead_reckon(model_cfg(m), w, s, f)
    return r


@functools.lru_cache(maxsize=None)
def golden_window():
    from cerberus_amd import synth
    return synth.make_window(synth.default_config(), n_landmarks=24, seed=5)


@functools.lru_cache(maxsize=None)
def tie_inputs():
    """(tag, model, samples of an interval with its constructor sample first, lin, the pinned record or None) for the ten intervals of the
    golden window on the contact inputs of tests/golden/make_golden_edges.py: the reference's own records for models 0 and 2
    (preint_contact_edges.npz), the oracle's for all three"""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_edges as E
    ge = np.load(os.path.join(ROOT, "tests", "golden", "preint_contact_edges.npz"))
    w = golden_window()
    ce = E.contact_edges(w.samples, w.sample_offsets, seed=int(ge["flag_seed"]))
    fe = E.force_edges(w.samples, w.sample_offsets, seed=int(ge["force_seed"]))
    out = []
    for m, smp, gold in ((0, ce, ge["flags"]), (1, ce, None), (2, fe, ge["force"])):
        for k in range(w.F - 1):
            out.append(("model %d interval %d" % (m, k), m, smp[w.sample_offsets[k]:w.sample_offsets[k + 1]], np.array(w.lin[k]), None if gold is None else gold[k]))
    return out


def _record_parts(rec):
    return np.concatenate([rec[4:8], rec[8:11], rec[11:23]])   # delta_q x y z w, delta_v, delta_eps


def _model_parts(r):
    return np.concatenate([[r["dq"][1], r["dq"][2], r["dq"][3], r["dq"][0]], r["dv"], np.asarray(r["eps"]).ravel()]).astype(np.float64)


def _parts_error(got, ref):
    return max(L._err(got[0:4], ref[0:4]), L._err(got[4:7], ref[4:7]), L._err(got[7:19], ref[7:19]))


def test_fp64_floor_measured():
    """The floor: the definition in float64 against the same in numpy.longdouble, over every case and every tie input. Printed per
    group; leg_dr_model.FLOOR must cover the largest and be no loose cover."""
    assert np.finfo(np.longdouble).eps < 1e-18   # the floor needs a long double wider than double
    worst = {}
    for case in cases():
        tag, m, w, s, f = case
        r = reference(case)
        assert r.status == L.OK, tag
        x = L.window_leg_dead_reckon(model_cfg(m), w, s, f, dtype=np.longdouble)
        assert L.flags_of((x.state, x.legs, x.trajectory)).tobytes() == L.flags_of((r.state, r.legs, r.trajectory)).tobytes(), tag
        for k, e in L.group_errors((x.state, x.legs, x.trajectory), (r.state, r.legs, r.trajectory)).items():
            worst[k] = max(worst.get(k, 0.0), e)
    tie = 0.0
    for tag, m, s, lin, _ in tie_inputs():
        a, b = L.integrate(model_cfg(m), lin, s), L.integrate(model_cfg(m), lin, s, np.longdouble)
        tie = max(tie, _parts_error(_model_parts(a), _model_parts(b)))
    print("MEASURED floor per group: %s; tie inputs (dq dv eps) %.1e" % (", ".join("%s %.1e" % kv for kv in sorted(worst.items())), tie))
    top = max(max(worst.values()), tie)
    print("MEASURED floor %.2e (leg_dr_model.FLOOR %.0e, tolerance %.0e)" % (top, L.FLOOR, L.TOL))
    assert top <= L.FLOOR
    assert top >= 0.25 * L.FLOOR   # (the constant is what is measured, not a loose cover)
    assert L.TOL == 10 * L.FLOOR


def test_branch_inputs_sit_where_claimed():
    for tag, m, w, s, f, what in branch_cases():
        r = L.window_leg_dead_reckon(model_cfg(m), w, s, f)
        assert r.status == L.OK and r.n_steps == 11, tag
        if what == "all_air":
            assert r.branches["all_air"] == r.n_steps and not r.branches["flags"].any(), tag
            # and the fused position still moves: the weights are the in-the-air ones, equal for the four legs
            assert np.abs(r.state[L.S_SUM_EPS]).max() > 0 and np.ptp(r.trajectory[:, L.T_W].reshape(-1, 4, 3), axis=1).max() == 0, tag
        elif what == "clamped":
            assert r.branches["clamped"] > 0 and (r.trajectory[:, L.T_W].reshape(-1, 4, 3)[:, 1] == 0.001).any(), tag
            assert (r.trajectory[:, L.T_W].reshape(-1, 4, 3)[:, 0] > 0.001).all(), tag   # (the other legs are not clamped)
        else:
            fl = r.branches["flags"][:, 1]
            assert fl[0] == 1.0 and fl[-1] == 0.0 and set(fl) == {0.0, 1.0}, (tag, fl)
    # contact model 2 reaches both values of the truncated flag on the gait's forces, and wraps the window
    w = kind_window("L9", 1)
    r = L.window_leg_dead_reckon(model_cfg(2), w, forces(take(w, 12, 2), 1))
    assert set(r.branches["flags"].ravel()) == {0.0, 1.0}


def test_tie_to_the_pinned_preintegration():
    """delta_q, delta_v and delta_eps of the definition at the same samples and linearisation point against the oracle's record (pinned
    against the reference's sources at 1e-12) under the three contact models, and against the reference's own records of the contact
    edge inputs (models 0 and 2), within the tolerance."""
    from oracle import oracle_py as O
    worst_o = worst_g = 0.0
    for tag, m, s, lin, gold in tie_inputs():
        ocfg = O.config_from(model_cfg(m))
        got = _model_parts(L.integrate(model_cfg(m), lin, s))
        rec = O.preintegrate_imu_leg(ocfg, s, lin)
        e = _parts_error(got, _record_parts(rec))
        worst_o = max(worst_o, e)
        assert e <= L.TOL, (tag, "oracle", e)
        assert abs(rec[0] - L.integrate(model_cfg(m), lin, s)["sum_dt"]) <= L.TOL
        if gold is not None:
            e = _parts_error(got, _record_parts(gold))
            worst_g = max(worst_g, e)
            assert e <= L.TOL, (tag, "reference record", e)
    print("MEASURED tie: to the oracle's records %.1e, to the reference's records %.1e (tolerance %.0e)" % (worst_o, worst_g, L.TOL))


def test_statuses_of_the_definition():
    w, two = kind_window("L9", 1), frames_window(2)
    cfg = model_cfg(0)
    s = take(w, 12, 0)
    for n in (0, 1):
        r = L.window_leg_dead_reckon(cfg, w, s[:n])
        assert (r.status, r.n_steps) == (L.OK, 0) and r.trajectory.shape == (0, L.TRAJ)
        assert not r.state[:1].any() and list(r.state[L.S_DQ]) == [0, 0, 0, 1] and not r.state[5:23].any() and not r.state[26:].any()
        assert r.state[L.S_POS].tobytes() == w.pose[w.F - 1, :3].tobytes() and (r.legs == w.pose[w.F - 1, :3]).all()
    r = L.window_leg_dead_reckon(cfg, two, s, 5)
    assert r.status == L.NO_FRAME and r.n_steps == 11 and not r.state.any() and not r.legs.any() and not r.trajectory.any()
    assert L.window_leg_dead_reckon(cfg, two, s, 1).status == L.OK
    for arr, idx in (("pose", (w.F - 1, 1)), ("pose", (w.F - 1, 5)), ("speed_bias", (w.F - 1, 4)), ("speed_bias", (w.F - 1, 7)), ("leg_bias", (w.F - 1, 2))):
        bad = w.twin()
        getattr(bad, arr)[idx] = np.nan
        r = L.window_leg_dead_reckon(cfg, bad, s)
        assert r.status == L.NUMERIC and not r.state.any() and not r.trajectory.any() and r.n_steps == 11, (arr, idx)
        assert L.window_leg_dead_reckon(cfg, bad, s, 3).status == L.OK   # (another frame's)
    bad = w.twin()
    bad.speed_bias[w.F - 1, 1] = np.nan   # the velocity is not read
    assert L.window_leg_dead_reckon(cfg, bad, s).status == L.OK
    for col in (0, 2, 5, 9, 25, 33):
        sn = s.copy()
        sn[7, col] = np.inf
        assert L.window_leg_dead_reckon(cfg, w, sn).status == L.NUMERIC, col
    sn = s.copy()
    sn[0, 0] = np.nan   # the first sample's dt is not read
    a, b = L.window_leg_dead_reckon(cfg, w, sn), L.window_leg_dead_reckon(cfg, w, s)
    assert a.status == L.OK and a.state.tobytes() == b.state.tobytes() and a.trajectory.tobytes() == b.trajectory.tobytes()
    sn[0, 9] = np.nan   # everything else of it is
    assert L.window_leg_dead_reckon(cfg, w, sn).status == L.NUMERIC
    assert L.window_leg_dead_reckon(cfg, w, sn[:1]).status == L.OK   # (without a step no sample is read)


# ------------------------------------------------------------------------------ the CPU path of legdr_host.hpp, in a sanitized program
@pytest.fixture(scope="module")
def host_program(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("leg_dr") / "leg_dr_check")
    src = os.path.join(ROOT, "tests", "host_check", "leg_dr_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", exe],
                   check=True, timeout=300)
    return exe


def run_host(exe, tmp, cfg, items):
    """items: (pose [7], speed_bias [9], leg_bias [4], samples [n, 35]) per window. Returns per window (status, n_steps, state, legs, ff, traj)."""
    cfg_d = np.frombuffer(bytes(cfg), dtype=np.float64)
    parts = [np.array([float(len(items))]), cfg_d]
    for pose, sb, lb, s in items:
        s = np.asarray(s, np.float64).reshape(-1, 35)
        parts += [np.array([float(len(s))]), np.asarray(pose, np.float64), np.asarray(sb, np.float64), np.asarray(lb, np.float64), s.ravel()]
    fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    np.concatenate(parts).tofile(fin)
    p = subprocess.run([exe, fin, fout], capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stdout.strip() == "ok", (p.returncode, p.stdout, p.stderr)
    o = np.fromfile(fout, dtype=np.float64)
    out, at = [], 0
    for _ in items:
        status, n_steps = int(o[at]), int(o[at + 1])
        at += 2
        state, legs, ff = o[at:at + 32], o[at + 32:at + 44].reshape(4, 3), o[at + 44:at + 80]
        at += 80
        traj = o[at:at + 48 * n_steps].reshape(n_steps, 48)
        at += 48 * n_steps
        out.append((status, n_steps, state, legs, ff, traj))
    assert at == len(o)
    return out


def test_host_program_self_checks_under_sanitizers(host_program):
    p = subprocess.run([host_program], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stdout, p.stderr)
    assert p.stdout.strip() == "ok", p.stdout


def check_against_definition(tag, got, ref, worst):
    """(status, n_steps, state, legs, trajectory) against the definition's LegDeadReckoned: flags exactly, everything else within TOL"""
    status, n_steps, state, legs, traj = got
    assert (status, n_steps) == (ref.status, ref.n_steps), tag
    assert L.flags_of((state, legs, traj)).tobytes() == L.flags_of((ref.state, ref.legs, ref.trajectory)).tobytes(), tag
    assert not state[30:].any() and (traj.size == 0 or not traj[:, 47].any()), tag
    errs = L.group_errors((state, legs, traj), (ref.state, ref.legs, ref.trajectory))
    for k, e in errs.items():
        worst[k] = max(worst.get(k, 0.0), e)
    assert max(errs.values()) <= L.TOL, (tag, errs)


def test_host_path_matches_the_definition(host_program, tmp_path):
    """legdr_step through the CPU path, under the sanitizers, on every case: flags exactly, everything else within the tolerance; a
    window's last trajectory row and the state without a trajectory are checked bit for bit by the program itself"""
    worst = {}
    for m in MODELS:
        mine = [c for c in cases() if c[1] == m]
        items = []
        for tag, _, w, s, f in mine:
            f = w.F - 1 if f == -1 else f
            items.append((w.pose[f], w.speed_bias[f], w.leg_bias[f], s))
        for case, (status, n_steps, state, legs, ff, traj) in zip(mine, run_host(host_program, str(tmp_path), model_cfg(m), items)):
            check_against_definition(case[0], (status, n_steps, state, legs, traj), reference(case), worst)
    print("MEASURED host program against the definition: %s (tolerance %.0e)" % (", ".join("%s %.1e" % kv for kv in sorted(worst.items())), L.TOL))


def test_host_path_statuses_and_filter(host_program, tmp_path):
    """NUMERIC: zero rows for the failing window alone; the contact-force filter the CPU path leaves is the oracle's object's (O_FF layout)"""
    from oracle import oracle_py as O
    w = kind_window("L9", 1)
    f = w.F - 1
    s = take(w, 12, 0)
    sn = s.copy()
    sn[7, 25] = np.nan
    lbn = w.leg_bias[f].copy()
    lbn[3] = np.inf
    res = run_host(host_program, str(tmp_path), model_cfg(2), [(w.pose[f], w.speed_bias[f], w.leg_bias[f], forces(s, 1)), (w.pose[f], w.speed_bias[f], w.leg_bias[f], sn),
                                                                (w.pose[f], w.speed_bias[f], lbn, s), (w.pose[f], w.speed_bias[f], w.leg_bias[f], forces(s, 1))])
    assert [r[0] for r in res] == [L.OK, L.NUMERIC, L.NUMERIC, L.OK] and [r[1] for r in res] == [11] * 4
    for r in res[1:3]:
        assert not r[2].any() and not r[3].any() and not r[5].any()
    for a, b in zip(res[0][2:], res[3][2:]):
        assert a.tobytes() == b.tobytes()
    # the filter after the tie inputs of contact model 2 against the oracle's
    items, want = [], []
    for tag, m, smp, lin, _ in tie_inputs():
        if m != 2:
            continue
        items.append((np.array([0, 0, 0, 0, 0, 0, 1.0]), np.concatenate([np.zeros(3), lin[:6]]), lin[6:10], smp))
        ff, out = np.zeros(36), np.zeros(O.PREINT_DOUBLES)
        sa, lina = np.ascontiguousarray(smp, dtype=np.float64), np.ascontiguousarray(lin, dtype=np.float64)
        dp = C.POINTER(C.c_double)
        O.lib().orc_preintegrate_imu_leg_ff(C.byref(O.config_from(model_cfg(2))), C.cast(sa.ctypes.data, C.POINTER(O.Sample)),
                                            C.cast(sa[1:].ctypes.data, C.POINTER(O.Sample)), C.c_int(len(sa) - 1), lina[0:3].ctypes.data_as(dp),
                                            lina[3:6].ctypes.data_as(dp), lina[6:10].ctypes.data_as(dp), ff.ctypes.data_as(dp),
                                            C.cast(out.ctypes.data, C.POINTER(O.Preint)))
        want.append((ff, out))
    worst = 0.0
    for (status, n_steps, state, legs, ff, traj), (off, rec) in zip(run_host(host_program, str(tmp_path), model_cfg(2), items), want):
        assert status == L.OK
        assert ff[32:36].tobytes() == off[32:36].tobytes()   # the window's index
        worst = max(worst, L._err(ff[0:4], off[0:4]), L._err(ff[4:8], off[4:8]), L._err(ff[8:12], off[8:12]), L._err(ff[12:32], off[12:32]))
        worst = max(worst, _parts_error(state[1:20], _record_parts(rec)))
    print("MEASURED host filter and record parts against the oracle's object: %.1e (tolerance %.0e)" % (worst, L.TOL))
    assert worst <= L.TOL


# ------------------------------------------------------------------------------ the wrapper and the header
def test_wrapper_options_need_no_device():
    from cerberus_amd import _ctypes as T
    from cerberus_amd import api
    o = api.leg_dead_reckon_opts()
    assert (o.from_frame, o.reserved) == (-1, 0)
    assert api.leg_dead_reckon_opts(3).from_frame == 3 and api.leg_dead_reckon_opts(T.MAX_FRAMES - 1).from_frame == T.MAX_FRAMES - 1
    for bad in (-2, T.MAX_FRAMES, 1.5):
        with pytest.raises(ValueError):
            api.leg_dead_reckon_opts(bad)
    assert api.LegDeadReckoning._fields == ("state", "legs", "trajectory", "step_offsets", "n_steps", "status")
    assert (T.LEG_DR_STATE, T.LEG_DR_LEGS, T.LEG_DR_TRAJ) == (L.STATE, L.LEGS, L.TRAJ)
    assert hasattr(api.Batch, "leg_dead_reckon") and hasattr(api.Context, "window_leg_dead_reckon")


def _header_struct(name):
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    end = hdr.index("} %s;" % name)
    body = hdr[hdr.rindex("typedef struct {", 0, end):end]
    return [ln.split(";")[0].split() for ln in body.splitlines()[1:] if ";" in ln]


def test_struct_sizes_match_the_header():
    from cerberus_amd import _ctypes as T
    for name, mirror in (("vilo_leg_dead_reckon_opts", T.LegDeadReckonOpts), ("vilo_window_leg_dead_reckon_record", T.WindowLegDeadReckonRecord)):
        fields = _header_struct(name)
        assert [f for f, _ in mirror._fields_] == [f[-1] for f in fields] and all(f[0] == "int32_t" for f in fields)
        assert C.sizeof(mirror) == 4 * len(fields) == 8
    hdr = open(os.path.join(ROOT, "include", "vilo_gpu.h")).read()
    assert "state_out[w][32]" in hdr and "legs_out[w][12]" in hdr and "[sum n_steps][48]" in hdr
    src = open(os.path.join(ROOT, "cerberus_amd", "csrc", "legdr_host.hpp")).read()
    for k, v in (("STATE", L.STATE), ("LEGS", L.LEGS), ("TRAJ", L.TRAJ), ("ROW", 35)):
        assert re.search(r"#define LEGDR_%s %d\b" % (k, v), src), k


def test_library_exports_the_entry_points():
    from cerberus_amd import _ctypes as T
    lib = C.CDLL(os.path.join(ROOT, "cerberus_amd", "lib", "libvilo_gpu.so"))
    for name in ("vilo_default_leg_dead_reckon_opts", "vilo_batch_leg_dead_reckon", "vilo_window_leg_dead_reckon", "vilo_last_leg_dead_reckon_ms"):
        assert hasattr(lib, name), name
    o = T.LegDeadReckonOpts(7, 7)
    lib.vilo_default_leg_dead_reckon_opts(C.byref(o))   # host code: needs no device
    assert (o.from_frame, o.reserved) == (-1, 0)
