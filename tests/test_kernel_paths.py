"""Every form of the Gauss-Newton iteration that a batch can take, against the oracle and against each other.

vilo::plan_solve (cerberus_amd/csrc/launch_plan.hpp; pinned on a CPU by tests/test_launch_plan.py) chooses the visual linearisation, the IMU
form, the bookkeeping + assembly and the solver from the batch size, the number of packed waves, the row form and switches the library reads
once per process; one batch size sees one combination. Each row below pins its switches in a subprocess of its own (tests/_paths_worker.py,
one after another), solves a fixed window set through a resident batch three times (plain launches, then replays of the captured sequence),
and asserts the descriptor vilo_debug_batch_path reports, so that no two rows run the same path by accident.

The window set: two bench windows (200 landmarks, prior), one without a prior, partial windows of 4 and 8 frames, one with interval 4
skipped, one without landmarks, one with 7 and one with 500 landmarks (multi-chunk groups), at the first, a middle and the last positions;
twins of the bench windows elsewhere. A second batch of two far-off windows with a huge trust region drives rejected steps through the
bookkeeping of each assembly form.

A third batch (worker spec "field") holds the windows of tests/field_windows.py, the shape a feature tracker hands over: tracks of any
length side by side in one packed wave, a quarter of the observations without a right-camera match, mismatches that stay on the Huber
branch, a landmark with one factor, a group of more than 64 lanes, one all-mono window, one partial one — the six windows in turn over 32
positions (rows A to L; the td-estimating one at position 6 of the 23-column rows) and over 257, 513 and 2049 positions (row N). The same
checks and bounds hold on them (tests/test_field_windows.py holds the properties of the windows on a CPU).

A fourth batch (worker spec "alt") holds the same field windows generated, filled and solved under the alternative configuration of
tests/alt_config.py, in every row that has the field batch: huber_delta, focal_length and g_norm travel as launch arguments of every
visual, cost and IMU kernel form, and at their defaults (1.0 among them) a wrong launch line is bitwise right. 32 positions per row; 257
and 2049 as well in row N, where the plan changes.

A fifth and a sixth batch (worker specs "const" and "vins") hold the windows of tests/const_windows.py: the block-constancy masks the
reference's estimator and the shipped configurations produce (extrinsics constant on every partial, slow or estimate_extrinsic: 0 window,
leg biases constant with a prior under optimize_leg_bias: 0, both, and the IMU-only windows of the vins configurations in batches of their
own), different masks side by side at every position. The mask is read by every visual family's landmark-coupling rows, by cd_active in
every assembly, solver and gradient kernel and by three hand-written copies of its predicate; under the default mask a wrong one is bitwise
invisible. On top of the field batches' checks every constant block of every returned state is bitwise the uploaded one
(tests/test_const_windows.py holds on a CPU that each flag moves the oracle's answer by 1000 bounds or more).

A seventh and an eighth batch (worker specs "frames" and "vframes") hold the windows of tests/frame_windows.py: one window for every frame
count from 2 to 11 (the batches above solve 4, 8 and 11), leg and IMU-only windows apart, four different frame counts in every aligned
group of four positions, 2 frames beside 11 and 10. The frame count decides where the 6F-wide pose system ends inside its 16-column
tiles, the parity of the loops over frames, the blocks every assembly pads and where a window joins the four-windows-per-wave chain
factorisation. On top of the const batches' checks the state rows of the absent frames come back bytewise as uploaded, which is what
include/vilo_gpu.h promises of vilo_batch_download (tests/test_frame_windows.py holds the windows' properties on a CPU).

Checks: every special window at every position against the oracle (equal iterations / successful steps, cost 1e-8, states 1e-8; the
far-off windows: equal decisions, states 1e-4 as tests/test_solver_forms.py holds the solver forms); bitwise where the code or the
documents claim it; 1e-9 elsewhere on the windows with a prior (the solver forms' bound)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_C = {"VILO_SMALL_FUSE_MAX_WINDOWS": "0"}
_E = {"VILO_ASM_SMALL_MAX_WINDOWS": "0"}
_F = dict(_E, VILO_NO_TPAR="1")
_G = dict(_F, VILO_SMALL_FUSE_MAX_WINDOWS="0", VILO_IMU_SINGLE_MAX_WINDOWS="0", VILO_SOLVER="split")
SIZES = [128, 129, 256, 257, 512, 513, 1024, 1025, 2048, 2049]

# row: (environment, worker spec)
ROWS = {
    "A": ({}, {"far": 1, "host": 1, "field": 1, "alt": 1}),
    "B1": ({"VILO_NO_TPAR": "1", "VILO_IMU_FIRST": "1"}, {"far": 1, "field": 1, "alt": 1}),
    "B0": ({"VILO_NO_TPAR": "1", "VILO_IMU_FIRST": "0"}, {"far": 1, "field": 1, "alt": 1}),
    "C": (_C, {"far": 1, "field": 1, "alt": 1}),
    "D": (dict(_C, VILO_IMU_SINGLE_MAX_WINDOWS="0"), {"far": 1, "field": 1, "alt": 1}),
    "E": (_E, {"far": 1, "field": 1, "alt": 1}),
    "F": (_F, {"far": 1, "field": 1, "alt": 1}),
    "G": (_G, {"far": 1, "field": 1, "alt": 1}),
    "H": (dict(_G, VILO_VISUAL_FORM="single"), {"far": 1, "field": 1, "alt": 1}),
    "Itpar": ({}, {"compact": 0, "far": 1, "field": 1, "alt": 1}),
    "Iwalk": ({"VILO_NO_TPAR": "1"}, {"compact": 0, "far": 1, "field": 1, "alt": 1}),
    "J": ({}, {"td": 1, "field": 1, "alt": 1}),
    "K0": ({"VILO_NO_TPAR": "1", "VILO_WAVE_ORDER": "0"}, {"field": 1, "alt": 1}),
    "K1": ({"VILO_NO_TPAR": "1", "VILO_WAVE_ORDER": "1"}, {"field": 1, "alt": 1}),
    "K2": ({"VILO_NO_TPAR": "1", "VILO_WAVE_ORDER": "2"}, {"field": 1, "alt": 1}),
    "L": ({"VILO_NO_GRAPH": "1"}, {"field": 1, "alt": 1}),
    "M": ({"VILO_FULL_RECORD_UPLOAD": "1", "VILO_NO_PINNED_STAGING": "1"}, {"host_only": 1}),
    "N": ({}, {"sizes": SIZES, "few_sizes": [300], "field": 1, "alt": 1, "field_sizes": [257, 513, 2049], "alt_sizes": [32, 257, 2049]}),
}
FIELD_ROWS = [r for r in ROWS if "field" in ROWS[r][1]]
# the windows of tests/const_windows.py: "const" in every row that has the field batch, "vins" (IMU-only) in these rows — each IMU form, each
# assembly, each solver, both visual families and both row widths. They ride in the rows' own workers; row N's sizes in a worker of
# their own under the same (empty) environment, which keeps row N's worker inside its time limit.
CONST_ROWS = FIELD_ROWS
VINS_ROWS = ["A", "B0", "C", "D", "E", "G", "H", "Itpar", "J", "N"]
for _r in CONST_ROWS:
    if _r != "N":
        ROWS[_r][1]["const"] = 1
        if _r in VINS_ROWS:
            ROWS[_r][1]["vins"] = 1
        ROWS[_r][1]["frames"] = 1   # the windows of tests/frame_windows.py, likewise (row N's sizes: the worker "Nframes")
        if _r in VINS_ROWS:
            ROWS[_r][1]["vframes"] = 1
N_SIZES = [32, 257, 513, 2049]
FRAMES_N_SIZES = [257, 513, 2049]
ALONE = ("c40_ex", "c40_lb", "c60_partial8")
FRAMES_ALONE = ("g2", "g3", "g10")
EXTRA_RUNS = {
    "Nframes": ({}, {"sizes": [], "frames": 1, "vframes": 1, "frames_sizes": FRAMES_N_SIZES, "vframes_sizes": FRAMES_N_SIZES}),
    "Aframes_alone": ({}, {"sizes": [], "frames_alone": list(FRAMES_ALONE)}),
    "Nconst": ({}, {"sizes": [], "const": 1, "vins": 1, "const_sizes": N_SIZES, "vins_sizes": N_SIZES}),
    "Aalone": ({}, {"sizes": [], "const_alone": list(ALONE)}),
}
FIELD_PRIOR = ("f40", "f200", "f70_chunks", "f40_allmono")   # the field windows with a prior and compact rows: the 1e-9 bound between forms


def _p(visual, imu, imu_order, assembly, solver, rows="compact"):
    return dict(visual=visual, imu=imu, imu_order=imu_order, assembly=assembly, solver=solver, rows=rows)


SMALL = _p("small_c", "fused", "first", "small", "mw8")
PC_SMALL = _p("pc_imu", "fused", "first", "small", "mw8")
EXPECT = {
    "A": SMALL, "L": SMALL,
    "B1": PC_SMALL, "K0": PC_SMALL, "K1": PC_SMALL, "K2": PC_SMALL,
    "B0": _p("pc_imu", "fused", "last", "small", "mw8"),
    "C": _p("tpar_c", "single", "none", "small", "mw8"),
    "D": _p("tpar_c", "pair", "none", "small", "mw8"),
    "E": _p("tpar_c", "single", "none", "full", "mw8"),
    "F": _p("pc_imu", "fused", "first", "full", "mw8"),
    "G": _p("pc", "pair", "none", "full", "split"),
    "H": _p("single_c", "pair", "none", "full", "split"),
    "Itpar": _p("tpar", "single", "none", "accept_wave", "mw8", "full"),
    "Iwalk": _p("single", "single", "none", "accept_wave", "mw8", "full"),
    "J": _p("tpar", "single", "none", "accept_wave", "mw8", "full"),
    # row N: the natural thresholds (VILO_ASM_SMALL_MAX_WINDOWS 256, VILO_MW8_MAX_WINDOWS 512, VILO_SPLIT_MIN_WINDOWS 1025,
    # VILO_SMALL_FUSE_MAX_WINDOWS 2048; IMU workgroups first up to 256 windows) — every such batch has more than 256 packed waves
    "128": PC_SMALL, "129": PC_SMALL, "256": PC_SMALL,
    "257": _p("pc_imu", "fused", "last", "full", "mw8"), "512": _p("pc_imu", "fused", "last", "full", "mw8"),
    "513": _p("pc_imu", "fused", "last", "full", "wave"), "1024": _p("pc_imu", "fused", "last", "full", "wave"),
    "1025": _p("pc_imu", "fused", "last", "full", "split"), "2048": _p("pc_imu", "fused", "last", "full", "split"),
    "2049": _p("pc", "pair", "none", "full", "split"),   # the bench's kernel set
    # 300 windows of a few landmarks: at most 256 packed waves beyond the small assembly
    "few300": _p("tpar_c", "pair", "none", "full", "mw8"),
}
WAVE_ORDER = {"K0": 0, "K2": 2}
PRIOR = ("bench0", "bench1", "skip4", "no_lm", "lm7", "lm500")   # well-conditioned: the 1e-9 bound between forms
_cache = {}


def _run(row):
    if row not in _cache:
        env_row, spec = ROWS[row] if row in ROWS else EXTRA_RUNS[row]
        env = {k: v for k, v in os.environ.items() if not k.startswith("VILO_") or k == "VILO_GPU_LIB"}
        env.update(env_row)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_paths_worker.py"), json.dumps(spec)], cwd=ROOT, env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, (row, p.stderr[-3000:])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("PATHS_JSON ")][-1]
        _cache[row] = json.loads(line[len("PATHS_JSON "):])
    return _cache[row]


def _sized(row):
    """(name, result of one batch) of a row: its W = 32 batch, or row N's sizes."""
    r = _run(row)
    return [(k, v) for k, v in r.items() if k != "far" and not k.startswith(("field", "alt", "const", "vins", "frames", "vframes"))]


def _field(row):
    """(name, result) of a row's field batches: "field32", or row N's three sizes."""
    return [(k, v) for k, v in _run(row).items() if k.startswith("field")]


@pytest.fixture(scope="module")
def oracle():
    """The oracle's solve of every special window, the td-estimating window and the far-off windows (the same records the worker builds)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _paths_worker as P
    from cerberus_amd import synth
    from oracle import oracle_py as O
    cfg = synth.default_config()
    ocfg = O.config_from(cfg)
    out = {}
    wins = dict(P.specials(cfg, ocfg), td=P.td_window(cfg, ocfg))
    for name, w in wins.items():
        s = O.solve_window(ocfg, w, O.default_opts(True, P.ITERS))
        out[name] = (s, [a.copy() for a in w.state_arrays()], w.F)
    for name, w in P.far_windows(cfg, ocfg).items():
        o = O.default_opts(True, P.FAR_ITERS)
        o.initial_trust_region_radius = 1e8
        s = O.solve_window(ocfg, w, o)
        out[name] = (s, [a.copy() for a in w.state_arrays()], w.F)
    out["_names"] = list(wins)[:-1]
    return out


def _rel_states(a_list, b_list, F=11):
    """max over the state arrays of |a - b| / max(1, |b|) (partial windows: the first F frames of the per-frame arrays)."""
    worst = 0.0
    for i, (a, b) in enumerate(zip(a_list, b_list)):
        a, b = np.asarray(a, float), np.asarray(b, float)
        if a.size == 0:
            continue
        if i < 3:   # (pose, speed_bias, leg_bias: per frame)
            a, b = a[:F], b[:F]
        worst = max(worst, float(np.abs(a - b).max() / max(1.0, np.abs(b).max())))
    return worst


def _specials_of(res, names):
    """{(name, block): (state arrays, summary)} of one batch's first solve."""
    s0 = res["solves"][0]
    out = {}
    for bi, block in enumerate(res["positions"]):
        for p, nm in zip(block, names):
            out[(nm, bi)] = (s0["state"][str(p)], s0["summ"][p])
    return out


@pytest.mark.parametrize("row", list(ROWS))
def test_descriptor(row):
    """vilo_debug_batch_path reports the row's forms; the first solve is plain launches, the later ones replays (VILO_NO_GRAPH: none)."""
    for name, res in _sized(row):
        if "solves" not in res:
            continue   # (row M: Context.solve_windows; no resident batch)
        exp = EXPECT[row if row != "N" else name]
        for i, s in enumerate(res["solves"]):
            got = dict(s["path"])
            replay, wo = got.pop("replay"), got.pop("wave_order")
            assert got == exp, (row, name, i, got)
            assert replay == (i > 0 and row != "L"), (row, name, i)
            assert wo == WAVE_ORDER.get(row, 1)
    if "far" in _run(row):
        for s in _run(row)["far"]["solves"]:
            got = dict(s["path"]); got.pop("replay"); got.pop("wave_order")
            assert got == EXPECT[row], (row, "far", got)


@pytest.mark.parametrize("row", list(ROWS))
def test_every_special_window_against_the_oracle(row, oracle):
    names = oracle["_names"]
    worst = worst_c = 0.0
    for name, res in _sized(row):
        if "solves" in res:
            sp = _specials_of(res, names)
        else:
            sp = {}
            for bi, block in enumerate(res["positions"]):
                for p, nm in zip(block, names):
                    sp[(nm, bi)] = (None, res["host"]["summ"][p])
        for (nm, bi), (st, sm) in sp.items():
            so, ost, F = oracle[nm]
            assert (sm["iterations"], sm["successful"]) == (so.iterations, so.num_successful), (row, name, nm, bi)
            np.testing.assert_allclose(sm["final_cost"], so.final_cost, rtol=1e-8, err_msg="%s %s %s %d" % (row, name, nm, bi))
            worst_c = max(worst_c, abs(sm["final_cost"] / so.final_cost - 1))
            if st is not None:
                e = _rel_states(st, ost, F)
                assert e < 1e-8, (row, name, nm, bi, e)
                worst = max(worst, e)
        if row == "J":
            so, ost, F = oracle["td"]
            p = len(names)
            e = _rel_states(res["solves"][0]["state"][str(p)], ost)
            sm = res["solves"][0]["summ"][p]
            assert (sm["iterations"], sm["successful"]) == (so.iterations, so.num_successful)
            np.testing.assert_allclose(sm["final_cost"], so.final_cost, rtol=1e-8)
            assert e < 1e-8, ("td window", e)
            worst = max(worst, e)
    far_e = None
    if "far" in _run(row):
        far_e = 0.0
        s0 = _run(row)["far"]["solves"][0]
        for i, nm in enumerate(("far42", "far51")):
            so, ost, F = oracle[nm]
            sm = s0["summ"][i]
            assert (sm["iterations"], sm["successful"]) == (so.iterations, so.num_successful), (row, nm)
            assert sm["successful"] + 2 <= sm["iterations"]   # (rejected steps happened)
            far_e = max(far_e, _rel_states(s0["state"][str(i)], ost))
        assert far_e < 1e-4, (row, far_e)
    print("MEASURED test_kernel_paths[%s] vs oracle: states %.2e, cost %.2e, far-off states %s" % (row, worst, worst_c, "-" if far_e is None else "%.2e" % far_e))


@pytest.mark.parametrize("row", [r for r in ROWS if r != "M"])
def test_replays_are_bitwise_the_first_solve(row):
    for name, res in _sized(row) + ([("far", _run(row)["far"])] if "far" in _run(row) else []):
        s = res["solves"]
        for i in (1, 2):
            assert s[i]["digest"] == s[0]["digest"] and s[i]["summ"] == s[0]["summ"], (row, name, i)


def _same(a, b, with_summaries=True, skip=(), key="32"):
    ra, rb = _run(a)[key], _run(b)[key]
    da = ra["solves"][0] if "solves" in ra else ra["host"]
    db = rb["solves"][0] if "solves" in rb else rb["host"]
    diff = [p for p, (x, y) in enumerate(zip(da["digest"], db["digest"])) if x != y and p not in skip]
    assert not diff, (a, b, "states differ at positions", diff)
    if with_summaries:
        assert [s for p, s in enumerate(da["summ"]) if p not in skip] == [s for p, s in enumerate(db["summ"]) if p not in skip], (a, b)
    else:
        for sa, sb in zip(da["summ"], db["summ"]):
            assert (sa["iterations"], sa["successful"]) == (sb["iterations"], sb["successful"])
            np.testing.assert_allclose(sa["cost_trace"], sb["cost_trace"], rtol=1e-11)
    if key == "32" and "far" in _run(a) and "far" in _run(b):
        fa, fb = _run(a)["far"]["solves"][0], _run(b)["far"]["solves"][0]
        assert fa["digest"] == fb["digest"], (a, b, "far")


@pytest.mark.parametrize("a,b", [("B0", "B1"), ("C", "A"), ("D", "A"), ("H", "G"), ("K0", "B1"), ("K1", "B1"), ("K2", "B1"),
                                 ("L", "A")])
def test_bitwise_pairs(a, b):
    """IMU workgroups first or last; the fused and the separate IMU forms (imu_fused_body: "bitwise the same Gram"); the one-wave and the
    producer / consumer compact visual forms; the launch order of the packed waves; plain launches instead of replays."""
    _same(a, b)


def test_frame_parallel_and_walking_forms_give_the_same_states():
    """k_lin_small_c and k_visual_linearize_pc_imu (both with k_assemble_s and the eight-wave solver): the same states bit for bit; the
    visual cost's partial sums are added in another order, so the summaries agree to rounding."""
    _same("B1", "A", with_summaries=False)


def test_host_hand_over_switches():
    """VILO_FULL_RECORD_UPLOAD / VILO_NO_PINNED_STAGING through Context.solve_windows: bitwise the default hand-over's answer, which is
    bitwise the resident batch's."""
    _same("M", "A")
    ra = _run("A")["32"]
    assert ra["host"]["digest"] == ra["solves"][0]["digest"] and ra["host"]["summ"] == ra["solves"][0]["summ"]


def test_one_td_estimating_window_sends_the_batch_to_23_columns():
    """Row J is row I (23-column rows) plus one td-estimating window at the first pad position: every other window bitwise row I's."""
    _same("J", "Itpar", skip=(9,))


def test_the_bench_kernel_set_at_small_and_full_size(oracle):
    """Row G (the 32 768-window launch's kernel set pinned at 32 windows) and the natural 2049-window batch: the special windows bitwise."""
    g = _specials_of(_run("G")["32"], oracle["_names"])
    n = _specials_of(_run("N")["2049"], oracle["_names"])
    for k in g:
        assert g[k] == n[k], k


@pytest.mark.parametrize("row", ["B0", "E", "F", "G", "Itpar", "Iwalk", "N"])
def test_other_forms_agree_with_row_A_to_rounding(row, oracle):
    """Where no bitwise claim exists: 1e-9 relative on the windows with a prior (the bound tests/test_solver_forms.py holds between
    solver forms), equal decisions everywhere."""
    names = oracle["_names"]
    ref = _specials_of(_run("A")["32"], names)
    worst = 0.0
    for name, res in _sized(row):
        sp = _specials_of(res, names)
        for (nm, bi), (st, sm) in sp.items():
            st_a, sm_a = ref[(nm, 0)]
            assert (sm["iterations"], sm["successful"]) == (sm_a["iterations"], sm_a["successful"]), (row, name, nm, bi)
            if nm in PRIOR:
                e = _rel_states(st, st_a)
                assert e < 1e-9, (row, name, nm, bi, e)
                np.testing.assert_allclose(sm["cost_trace"], sm_a["cost_trace"], rtol=1e-9)
                worst = max(worst, e)
    far_e = None
    if "far" in _run(row):
        far_e = 0.0
        fa, fr = _run("A")["far"]["solves"][0], _run(row)["far"]["solves"][0]
        for i in (0, 1):
            assert (fr["summ"][i]["iterations"], fr["summ"][i]["successful"]) == (fa["summ"][i]["iterations"], fa["summ"][i]["successful"])
            far_e = max(far_e, _rel_states(fr["state"][str(i)], fa["state"][str(i)]))
        assert far_e < 1e-4, far_e
    print("MEASURED test_kernel_paths[%s] vs row A: states %.2e (windows with a prior), far-off %s" % (row, worst, "-" if far_e is None else "%.2e" % far_e))


# ---- the field windows (tests/field_windows.py): the same rows, the shape a feature tracker hands over ----
@pytest.fixture(scope="module")
def field_oracle():
    """The oracle's solve of every field window, once: {name: (summary, state arrays, F)}."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _paths_worker as P
    import field_windows as FW
    from cerberus_amd import synth
    from oracle import oracle_py as O
    cfg = synth.default_config()
    ocfg = O.config_from(cfg)
    out = {}
    for name, w in FW.field_set(cfg, ocfg).items():
        s = O.solve_window(ocfg, w, O.default_opts(True, P.ITERS))
        out[name] = (s, [a.copy() for a in w.state_arrays()], w.F)
    return out


def _field_by_name(res):
    """{name: [(position, state arrays or None, summary)]} of a field batch's first solve."""
    s0 = res["solves"][0]
    out = {}
    for p, nm in enumerate(res["names"]):
        out.setdefault(nm, []).append((p, s0["state"].get(str(p)), s0["summ"][p]))
    return out


@pytest.mark.parametrize("row", FIELD_ROWS)
def test_field_descriptor(row):
    """The field batch takes the row's forms (row N: the three sizes' entries), the first solve plain launches, the later ones replays."""
    got_keys = [k for k, _ in _field(row)]
    assert got_keys == (["field257", "field513", "field2049"] if row == "N" else ["field32"]), got_keys
    for name, res in _field(row):
        exp = EXPECT[row if row != "N" else str(res["W"])]
        assert len(res["names"]) == res["W"]
        assert ("f40_td" in res["names"]) == (row in ("J", "Itpar", "Iwalk"))
        for i, s in enumerate(res["solves"]):
            got = dict(s["path"])
            replay, wo = got.pop("replay"), got.pop("wave_order")
            assert got == exp, (row, name, i, got)
            assert replay == (i > 0 and row != "L"), (row, name, i)
            assert wo == WAVE_ORDER.get(row, 1)


FIELD_NAMES = {"f40", "f200", "f130_noprior", "f70_chunks", "f40_allmono", "f60_partial8"}
TD_WINDOWS = ("f40_td", "c40_ex_td", "v40_td")   # one position only (6), and only among rows of 23 columns


def _check_field_batches(row, batches, oracle, need=FIELD_NAMES, edge=6, min_pos=3):
    """Every field window at every position of the batches [(name, result)]: the oracle's decisions, cost 1e-8, states 1e-8;
    each window at first, middle and last positions (within `edge` of either end: one turn of the six field windows; a batch of more
    windows in turn passes its own); one window, one answer wherever it sits; replays bitwise the plain launches.
    Returns the largest state and cost difference."""
    worst = worst_c = 0.0
    for name, res in batches:
        s = res["solves"]
        assert len(s) >= 2
        for i in range(1, len(s)):
            assert s[i]["digest"] == s[0]["digest"] and s[i]["summ"] == s[0]["summ"], (row, name, i)
        by_name = _field_by_name(res)
        assert set(by_name) >= set(need)
        for nm, entries in by_name.items():
            so, ost, F = oracle[nm][:3]
            if nm not in TD_WINDOWS:
                pos = [p for p, _, _ in entries]
                assert pos[0] < edge and pos[-1] >= res["W"] - edge and len(pos) >= min_pos, (row, name, nm, pos)   # first, middle and last positions
            n_states = 0
            for p, st, sm in entries:
                assert (sm["iterations"], sm["successful"]) == (so.iterations, so.num_successful), (row, name, nm, p)
                np.testing.assert_allclose(sm["final_cost"], so.final_cost, rtol=1e-8, err_msg="%s %s %s %d" % (row, name, nm, p))
                worst_c = max(worst_c, abs(sm["final_cost"] / so.final_cost - 1))
                assert s[0]["digest"][p] == s[0]["digest"][entries[0][0]] and sm == entries[0][2], (row, name, nm, p)
                if st is not None:
                    e = _rel_states(st, ost, F)
                    assert e < 1e-8, (row, name, nm, p, e)
                    worst = max(worst, e)
                    n_states += 1
            assert n_states >= min(3, len(entries)), (row, name, nm)
    return worst, worst_c


@pytest.mark.parametrize("row", FIELD_ROWS)
def test_field_windows_against_the_oracle(row, field_oracle):
    """Every field window at every position: the oracle's decisions, cost 1e-8, states 1e-8; one window, one answer
    wherever it sits in the batch; replays bitwise the plain launches."""
    assert all(len(res["solves"]) == 3 for _, res in _field(row))
    worst, worst_c = _check_field_batches(row, _field(row), field_oracle)
    print("MEASURED test_kernel_paths[%s] field windows vs oracle: states %.2e, cost %.2e" % (row, worst, worst_c))


@pytest.mark.parametrize("a,b", [("B0", "B1"), ("C", "A"), ("D", "A"), ("H", "G"), ("K0", "B1"), ("K1", "B1"), ("K2", "B1"), ("L", "A")])
def test_field_bitwise_pairs(a, b):
    """The pairs of test_bitwise_pairs, on the field batch."""
    _same(a, b, key="field32")


def test_field_frame_parallel_and_walking_forms_give_the_same_states():
    _same("B1", "A", with_summaries=False, key="field32")


def test_field_td_estimating_window_among_23_column_rows():
    """Rows J and Itpar run the same forms on the same field batch: bitwise on every window but the td-estimating one (position 6 of
    both), as test_bitwise_pairs' J / Itpar case leaves the td-estimating special out."""
    names = _run("J")["field32"]["names"]
    td = tuple(p for p, nm in enumerate(names) if nm == "f40_td")
    assert td == (6,) and names == _run("Itpar")["field32"]["names"]
    _same("J", "Itpar", skip=td, key="field32")


def test_field_bench_kernel_set_at_small_and_full_size():
    """Row G's field batch of 32 and row N's of 2049: each field window bitwise the same."""
    g, n = _field_by_name(_run("G")["field32"]), _field_by_name(_run("N")["field2049"])
    for nm in g:
        assert g[nm][0][1] is not None and g[nm][0][1:] == n[nm][0][1:], nm


@pytest.mark.parametrize("row", ["B0", "E", "F", "G", "Itpar", "Iwalk", "N"])
def test_field_other_forms_agree_with_row_A_to_rounding(row):
    """1e-9 relative on the field windows with a prior, equal decisions on every one."""
    ref = _field_by_name(_run("A")["field32"])
    worst = 0.0
    for name, res in _field(row):
        for nm, entries in _field_by_name(res).items():
            if nm not in ref:
                continue   # (the td-estimating window: rows of 23 columns only)
            _, st_a, sm_a = ref[nm][0]
            for p, st, sm in entries:
                assert (sm["iterations"], sm["successful"]) == (sm_a["iterations"], sm_a["successful"]), (row, name, nm, p)
                if nm in FIELD_PRIOR and st is not None:
                    e = _rel_states(st, st_a)
                    assert e < 1e-9, (row, name, nm, p, e)
                    np.testing.assert_allclose(sm["cost_trace"], sm_a["cost_trace"], rtol=1e-9)
                    worst = max(worst, e)
    print("MEASURED test_kernel_paths[%s] field windows vs row A: states %.2e (windows with a prior)" % (row, worst))


# ---- the field windows under the alternative configuration (tests/alt_config.py): every form's launch line carries sq, ha and gn ----
@pytest.fixture(scope="module")
def alt_oracle():
    """The oracle's solve of every field window generated and filled at the alternative configuration: {name: (summary, states, F)}."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _paths_worker as P
    import alt_config
    import field_windows as FW
    from cerberus_amd import synth
    from oracle import oracle_py as O
    acfg = alt_config.alt_config(synth.default_config())
    oacfg = O.config_from(acfg)
    out = {}
    for name, w in FW.field_set(acfg, oacfg).items():
        s = O.solve_window(oacfg, w, O.default_opts(True, P.ITERS))
        out[name] = (s, [a.copy() for a in w.state_arrays()], w.F)
    return out


def _alt(row):
    return [(k, v) for k, v in _run(row).items() if k.startswith("alt")]


@pytest.mark.parametrize("row", FIELD_ROWS)
def test_alt_config_field_windows_against_the_oracle(row, alt_oracle):
    """The alternative configuration's batch: the row's forms (row N: the natural ones of 32, 257 and 2049 windows), 1e-9 between forms on
    the windows with a prior (row A's batch of 32), and test_field_windows_against_the_oracle's checks through the same helper."""
    got_keys = [k for k, _ in _alt(row)]
    assert got_keys == (["alt32", "alt257", "alt2049"] if row == "N" else ["alt32"]), got_keys
    ref = _field_by_name(_run("A")["alt32"])
    worst_a = 0.0
    for name, res in _alt(row):
        exp = EXPECT[row] if row != "N" else (EXPECT["A"] if res["W"] == 32 else EXPECT[str(res["W"])])
        assert len(res["names"]) == res["W"]
        for i, sv in enumerate(res["solves"]):
            got = dict(sv["path"])
            replay, wo = got.pop("replay"), got.pop("wave_order")
            assert got == exp, (row, name, i, got)
            assert replay == (i > 0 and row != "L") and wo == WAVE_ORDER.get(row, 1), (row, name, i)
        for nm, entries in _field_by_name(res).items():
            if nm not in FIELD_PRIOR:
                continue
            _, st_a, sm_a = ref[nm][0]
            for p, st, sm in entries:
                if st is not None:
                    ea = _rel_states(st, st_a)
                    assert ea < 1e-9, (row, name, nm, p, ea)
                    np.testing.assert_allclose(sm["cost_trace"], sm_a["cost_trace"], rtol=1e-9)
                    worst_a = max(worst_a, ea)
    worst, worst_c = _check_field_batches(row, _alt(row), alt_oracle)
    print("MEASURED test_kernel_paths[%s] alternative configuration vs oracle: states %.2e, cost %.2e; vs row A %.2e; %.2f s of the row's worker"
          % (row, worst, worst_c, worst_a, sum(res["seconds"] for _, res in _alt(row))))


# ---- the block-constancy masks the reference produces (tests/const_windows.py): the same rows, leg and IMU-only batches ----
CONST_EDGE = {"const": 14, "vins": 6}   # within two turns of the seven leg windows (c40_ex_td displaces one first position), one of the five IMU-only


@pytest.fixture(scope="module")
def const_oracle():
    """The oracle's solve of every window of both sets, once: {name: (summary, state arrays, F, uploaded state arrays, indices of the
    constant ones)}."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _paths_worker as P
    import const_windows as CW
    from cerberus_amd import synth
    from oracle import oracle_py as O
    cfg = synth.default_config()
    ocfg = O.config_from(cfg)
    out = {}
    for name, w in list(CW.const_set(cfg, ocfg).items()) + list(CW.vins_set(cfg, ocfg).items()):
        init = w.clone_state()
        s = O.solve_window(ocfg, w, O.default_opts(True, P.ITERS))
        out[name] = (s, [a.copy() for a in w.state_arrays()], w.F, init, CW.constant_arrays(w))
    return out


def _const_run(row):
    return _run("Nconst" if row == "N" else row)


def _const(row, kind):
    """(name, result) of a row's "const" or "vins" batches: one of 32, or row N's four sizes."""
    return [(k, v) for k, v in _const_run(row).items() if k.startswith(kind)]


def _const_cases():
    return [(r, "const") for r in CONST_ROWS] + [(r, "vins") for r in VINS_ROWS]


def _const_need(kind):
    import const_windows as CW
    return CW.LEG_BATCH if kind == "const" else CW.VINS_BATCH


@pytest.mark.parametrize("row,kind", _const_cases())
def test_const_descriptor(row, kind):
    """Each batch takes the row's forms (row N: the entry of its size), the first solve plain launches, the later ones replays; the
    td-estimating window is in it exactly where the row runs 23-column rows."""
    got_keys = [k for k, _ in _const(row, kind)]
    assert got_keys == [kind + str(W) for W in (N_SIZES if row == "N" else [32])], got_keys
    for name, res in _const(row, kind):
        exp = EXPECT[row] if row != "N" else (EXPECT["A"] if res["W"] == 32 else EXPECT[str(res["W"])])
        assert len(res["names"]) == res["W"] and len(res["solves"]) == 3
        td = [p for p, nm in enumerate(res["names"]) if nm in TD_WINDOWS]
        assert td == ([6] if row in ("J", "Itpar", "Iwalk") else []), (row, name, td)
        for i, s in enumerate(res["solves"]):
            got = dict(s["path"])
            replay, wo = got.pop("replay"), got.pop("wave_order")
            assert got == exp, (row, name, i, got)
            assert replay == (i > 0 and row != "L"), (row, name, i)
            assert wo == WAVE_ORDER.get(row, 1)


def _check_constant_blocks(row, batches, oracle):
    """Every constant block of every returned state is bitwise the uploaded one: ex_pose / leg_bias / td per the window's mask, leg_bias of
    every IMU-only window (a back-substitution that writes a nonzero dx into a constant block, a predicate out of step with cd_active)."""
    n = 0
    for name, res in batches:
        for nm, entries in _field_by_name(res).items():
            _, _, _, init, const = oracle[nm]
            assert const and (2 in const or nm in ("c40_free", "c40_ex", "c200_ex", "c40_ex_td")), nm
            for p, st, _ in entries:
                if st is None:
                    continue
                for i in const:
                    assert np.array_equal(np.asarray(st[i], float).reshape(init[i].shape), init[i]), (row, name, nm, p, "state array %d moved" % i)
                    n += 1
    return n


@pytest.mark.parametrize("row,kind", _const_cases())
def test_const_windows_against_the_oracle(row, kind, const_oracle):
    """Every window of the set at every kept position: the oracle's decisions, cost 1e-8, states 1e-8; one window, one answer wherever it
    sits among other masks; replays bitwise the plain launches; constant blocks bitwise the uploaded ones; and, where no bitwise claim
    exists, row A's answer to rounding (test_const_other_forms_agree_with_row_A_to_rounding holds the bound)."""
    batches = _const(row, kind)
    worst, worst_c = _check_field_batches(row, batches, const_oracle, need=_const_need(kind), edge=CONST_EDGE[kind])
    n = _check_constant_blocks(row, batches, const_oracle)
    assert n >= sum(len(const_oracle[nm][4]) for nm in _const_need(kind)) * 3
    worst_a = _const_vs_row_A(row, kind, check=False)
    print("MEASURED test_kernel_paths[%s] %s windows vs oracle: states %.2e, cost %.2e; vs row A %.2e; %d constant blocks bitwise; %.2f s of the row's worker"
          % (row, kind, worst, worst_c, worst_a, n, sum(res["seconds"] for _, res in batches)))


def _const_vs_row_A(row, kind, check):
    """Largest state difference from row A's batch of 32 on the windows with a prior; check: equal decisions on every window, 1e-9 and
    cost_trace at rtol 1e-9 on those."""
    import const_windows as CW
    ref = _field_by_name(_run("A")[kind + "32"])
    worst = 0.0
    for name, res in _const(row, kind):
        for nm, entries in _field_by_name(res).items():
            if nm not in ref:
                continue   # (the td-estimating window: rows of 23 columns only)
            _, st_a, sm_a = ref[nm][0]
            for p, st, sm in entries:
                if check:
                    assert (sm["iterations"], sm["successful"]) == (sm_a["iterations"], sm_a["successful"]), (row, name, nm, p)
                if nm in CW.PRIOR_NAMES and st is not None:
                    e = _rel_states(st, st_a)
                    worst = max(worst, e)
                    if check:
                        assert e < 1e-9, (row, name, nm, p, e)
                        np.testing.assert_allclose(sm["cost_trace"], sm_a["cost_trace"], rtol=1e-9)
    return worst


@pytest.mark.parametrize("row,kind", [(r, k) for r, k in _const_cases() if r in ("B0", "E", "F", "G", "Itpar", "Iwalk", "N")])
def test_const_other_forms_agree_with_row_A_to_rounding(row, kind):
    """1e-9 relative on the windows with a prior (c40_*, c200_ex, v40, v40_ex, v40_skip), equal decisions on every one."""
    worst = _const_vs_row_A(row, kind, check=True)
    print("MEASURED test_kernel_paths[%s] %s windows vs row A: states %.2e (windows with a prior)" % (row, kind, worst))


_PAIRS = [("B0", "B1"), ("C", "A"), ("D", "A"), ("H", "G"), ("K0", "B1"), ("K1", "B1"), ("K2", "B1"), ("L", "A")]


@pytest.mark.parametrize("a,b,kind", [(a, b, "const") for a, b in _PAIRS] + [(a, b, "vins") for a, b in _PAIRS if a in VINS_ROWS and b in VINS_ROWS])
def test_const_bitwise_pairs(a, b, kind):
    """The pairs of test_bitwise_pairs, on the batches of mixed masks."""
    _same(a, b, key=kind + "32")


def test_const_frame_parallel_and_walking_forms_give_the_same_states():
    _same("B1", "A", with_summaries=False, key="const32")


@pytest.mark.parametrize("kind", ["const", "vins"])
def test_const_td_estimating_window_among_23_column_rows(kind):
    """Rows J and Itpar run the same forms on the same batch: bitwise on every window but the td-estimating one (position 6 of both)."""
    names = _run("J")[kind + "32"]["names"]
    td = tuple(p for p, nm in enumerate(names) if nm in TD_WINDOWS)
    assert td == (6,) and names == _run("Itpar")[kind + "32"]["names"]
    _same("J", "Itpar", skip=td, key=kind + "32")


@pytest.mark.parametrize("kind", ["const", "vins"])
def test_const_bench_kernel_set_at_small_and_full_size(kind):
    """Row G's batch of 32 and the natural one of 2049: each window bitwise the same."""
    g, n = _field_by_name(_run("G")[kind + "32"]), _field_by_name(_run("Nconst")[kind + "2049"])
    assert set(g) == set(n)
    for nm in g:
        assert g[nm][0][1] is not None and g[nm][0][1:] == n[nm][0][1:], nm


def test_const_window_alone_is_bitwise_the_window_among_other_masks():
    """c40_ex, c40_lb and c60_partial8 each in a batch of their own under row A's environment: states bitwise what they are inside
    const32, where the neighbours in the workgroup and in the packed-wave order carry other masks — no output depends on the
    batch a window shares."""
    alone = _run("Aalone")
    inside = _field_by_name(_run("A")["const32"])
    for nm in ALONE:
        s = alone["alone_" + nm]["solves"]
        assert s[1]["digest"] == s[0]["digest"] == s[2]["digest"]
        _, st, sm = inside[nm][0]
        assert st is not None and s[0]["state"]["0"] == st, nm
        sa = s[0]["summ"][0]
        assert (sa["iterations"], sa["successful"]) == (sm["iterations"], sm["successful"]), nm


# ---- every frame count from 2 to 11 (tests/frame_windows.py): the same rows, leg and IMU-only batches ----
# Between forms. These windows have no prior, so FIELD_PRIOR's 1e-9 does not apply: the bound is ten times the largest difference from row A
# measured on an MI355X over every row, size and window ("Every frame count"), and never above the 1e-8 that holds against the oracle.
FRAMES_BETWEEN_MEASURED = {"frames": 3.04e-10, "vframes": 3.83e-10}   # (rows G, H and N: the three-stage solver)
FRAMES_BETWEEN = {k: 1e-8 if v is None else min(1e-8, 10.0 * v) for k, v in FRAMES_BETWEEN_MEASURED.items()}


@pytest.fixture(scope="module")
def frames_oracle():
    """The oracle's solve of every window of both sets, once: {name: (summary, state arrays, F, uploaded state arrays, indices of the
    constant ones)}."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import _paths_worker as P
    import const_windows as CW
    import frame_windows as FR
    from cerberus_amd import synth
    from oracle import oracle_py as O
    cfg = synth.default_config()
    ocfg = O.config_from(cfg)
    out = {}
    for name, w in list(FR.leg_set(cfg, ocfg).items()) + list(FR.vins_set(cfg, ocfg).items()):
        init = w.clone_state()
        s = O.solve_window(ocfg, w, O.default_opts(True, P.ITERS))
        out[name] = (s, [a.copy() for a in w.state_arrays()], w.F, init, CW.constant_arrays(w))
    return out


def _frames(row, kind):
    """(name, result) of a row's "frames" or "vframes" batches: one of 32, or row N's three sizes (the worker "Nframes")."""
    return [(k, v) for k, v in _run("Nframes" if row == "N" else row).items() if k.startswith(kind)]


def _frames_cases():
    return [(r, "frames") for r in CONST_ROWS] + [(r, "vframes") for r in VINS_ROWS]


def _frames_need(kind):
    import frame_windows as FR
    return list(FR.LEG if kind == "frames" else FR.VINS)


@pytest.mark.parametrize("row,kind", _frames_cases())
def test_frames_descriptor(row, kind):
    """Each batch takes the row's forms (row N: the entry of its size), the first solve plain launches, the later ones replays, and is
    placed as frame_windows.batch_of places it."""
    import frame_windows as FR
    got_keys = [k for k, _ in _frames(row, kind)]
    assert got_keys == [kind + str(W) for W in (FRAMES_N_SIZES if row == "N" else [32])], got_keys
    order = FR.LEG_ORDER if kind == "frames" else FR.VINS_ORDER
    for name, res in _frames(row, kind):
        # row J takes 23-column rows because of its td-estimating window; these batches hold none, so there it runs row A's forms
        exp = EXPECT[str(res["W"])] if row == "N" else EXPECT["A" if row == "J" else row]
        assert res["names"] == [order[p % len(order)] for p in range(res["W"])] and len(res["solves"]) == 3
        for i, s in enumerate(res["solves"]):
            got = dict(s["path"])
            replay, wo = got.pop("replay"), got.pop("wave_order")
            assert got == exp, (row, name, i, got)
            assert replay == (i > 0 and row != "L"), (row, name, i)
            assert wo == WAVE_ORDER.get(row, 1)


def _check_absent_frames(row, batches, oracle):
    """include/vilo_gpu.h, vilo_batch_download: the rows at and beyond n_frames of pose, speed_bias and leg_bias are not written; they come
    back bytewise as uploaded. Returns the number of arrays compared."""
    n = 0
    for name, res in batches:
        for nm, entries in _field_by_name(res).items():
            _, _, F, init, _ = oracle[nm]
            for p, st, _ in entries:
                if st is None or F == 11:
                    continue
                for i in (0, 1, 2):
                    a = np.asarray(st[i], float)
                    assert a.shape == init[i].shape and a[F:].tobytes() == init[i][F:].tobytes(), (row, name, nm, p, "absent rows of state array %d" % i)
                    assert np.abs(init[i][F:]).max() > 0   # (the generator's later frames: not zeros a memset would also leave)
                    n += 1
    return n


def _frames_vs_row_A(row, kind, bound=None):
    """{window: largest state difference from row A's batch of 32}; bound: equal decisions, the states and the final cost within it. The
    costs along the way are printed, not held: after the first step an IMU-only window is still falling by orders of magnitude per step
    (v9: 4.5e7, 2.1e4, 80.5), and there two forms' costs differ by 1.6e-8 (measured, row Itpar) where their states differ by 1.4e-10."""
    ref = _field_by_name(_run("A")[kind + "32"])
    worst = {}
    for name, res in _frames(row, kind):
        for nm, entries in _field_by_name(res).items():
            _, st_a, sm_a = ref[nm][0]
            for p, st, sm in entries:
                if bound is not None:
                    assert (sm["iterations"], sm["successful"]) == (sm_a["iterations"], sm_a["successful"]), (row, name, nm, p)
                    np.testing.assert_allclose(sm["final_cost"], sm_a["final_cost"], rtol=bound)
                    worst["cost trace"] = max(worst.get("cost trace", 0.0), float(np.abs(np.array(sm["cost_trace"]) / np.array(sm_a["cost_trace"]) - 1).max()))
                if st is not None:
                    e = _rel_states(st, st_a)   # (all 11 rows: the absent frames' are the uploaded ones in both)
                    worst[nm] = max(worst.get(nm, 0.0), e)
                    if bound is not None:
                        assert e < bound, (row, name, nm, p, e)
    return worst


@pytest.mark.parametrize("row,kind", _frames_cases())
def test_frames_windows_against_the_oracle(row, kind, frames_oracle):
    """Every window of the set at every kept position: the oracle's decisions, cost 1e-8, states 1e-8; one window, one answer wherever it
    sits among other frame counts; replays bitwise the plain launches; constant blocks and the absent frames' rows bitwise the uploaded
    ones. Positions: the leg set has 16 windows, so a batch of 32 holds each at two positions (three each would take 48: min_pos is 2 for
    that batch alone); from 257 windows on, and in every IMU-only batch, each window sits at three positions or more, as the other
    batches' windows do."""
    batches = _frames(row, kind)
    worst = worst_c = 0.0
    for name, res in batches:
        # 16 leg windows over a pattern of 32 positions: two positions each in a batch of 32, the last ones inside the last 33 of a longer
        # one (a batch of 32 k + 1); the 7 IMU-only windows in turn
        edge, min_pos = (7, 3) if kind == "vframes" else ((16, 2) if res["W"] == 32 else (33, 3))
        e, c = _check_field_batches(row, [(name, res)], frames_oracle, need=_frames_need(kind), edge=edge, min_pos=min_pos)
        worst, worst_c = max(worst, e), max(worst_c, c)
    n = _check_constant_blocks(row, batches, frames_oracle)
    assert n >= sum(len(frames_oracle[nm][4]) for nm in _frames_need(kind)) * 2
    na = _check_absent_frames(row, batches, frames_oracle)
    assert na >= 3 * 2 * sum(frames_oracle[nm][2] < 11 for nm in _frames_need(kind))
    per_F = {}
    for name, res in batches:
        for nm, entries in _field_by_name(res).items():
            so, ost, F = frames_oracle[nm][:3]
            per_F[F] = max([per_F.get(F, 0.0)] + [_rel_states(st, ost, F) for _, st, _ in entries if st is not None])
    vs_a = _frames_vs_row_A(row, kind)
    print("MEASURED test_kernel_paths[%s] %s windows vs oracle: states %.2e, cost %.2e; per frame count %s; vs row A %.2e; %d constant blocks, %d absent-frame arrays bitwise; %.2f s of the row's worker"
          % (row, kind, worst, worst_c, " ".join("%d: %.1e" % (F, per_F[F]) for F in sorted(per_F)), max(vs_a.values()), n, na,
             sum(res["seconds"] for _, res in batches)))


@pytest.mark.parametrize("row,kind", [(r, k) for r, k in _frames_cases() if r in ("B0", "E", "F", "G", "Itpar", "Iwalk", "N")])
def test_frames_other_forms_agree_with_row_A_to_rounding(row, kind):
    """Where no bitwise claim exists: every window within FRAMES_BETWEEN of row A's answer in states and final cost, equal decisions."""
    worst = _frames_vs_row_A(row, kind, bound=FRAMES_BETWEEN[kind])
    trace = worst.pop("cost trace")
    print("MEASURED test_kernel_paths[%s] %s windows vs row A: states %.2e (bound %.1e), costs along the way %.1e; per window %s"
          % (row, kind, max(worst.values()), FRAMES_BETWEEN[kind], trace, " ".join("%s %.1e" % kv for kv in worst.items())))


@pytest.mark.parametrize("a,b,kind", [(a, b, "frames") for a, b in _PAIRS] + [(a, b, "vframes") for a, b in _PAIRS if a in VINS_ROWS and b in VINS_ROWS])
def test_frames_bitwise_pairs(a, b, kind):
    """The pairs of test_bitwise_pairs, on the batches of mixed frame counts."""
    _same(a, b, key=kind + "32")


def test_frames_frame_parallel_and_walking_forms_give_the_same_states():
    _same("B1", "A", with_summaries=False, key="frames32")


@pytest.mark.parametrize("kind", ["frames", "vframes"])
def test_frames_same_forms_in_two_rows_are_bitwise(kind):
    """Without a td-estimating window row J's batch takes row A's forms (test_frames_descriptor): bitwise on every window."""
    assert _run("J")[kind + "32"]["names"] == _run("A")[kind + "32"]["names"]
    _same("J", "A", key=kind + "32")


@pytest.mark.parametrize("kind", ["frames", "vframes"])
def test_frames_bench_kernel_set_at_small_and_full_size(kind):
    """Row G's batch of 32 and the natural one of 2049: each window bitwise the same."""
    g, n = _field_by_name(_run("G")[kind + "32"]), _field_by_name(_run("Nframes")[kind + "2049"])
    assert set(g) == set(n)
    for nm in g:
        assert g[nm][0][1] is not None and g[nm][0][1:] == n[nm][0][1:], nm


def test_frames_window_alone_is_bitwise_the_window_among_other_frame_counts():
    """The windows of 2, 3 and 10 frames each in a batch of their own under row A's environment: states bitwise what they are inside
    frames32, where the other windows of their aligned group of four run to 11 and 10 frames."""
    alone = _run("Aframes_alone")
    inside = _field_by_name(_run("A")["frames32"])
    for nm in FRAMES_ALONE:
        s = alone["falone_" + nm]["solves"]
        assert s[1]["digest"] == s[0]["digest"] == s[2]["digest"]
        _, st, sm = inside[nm][0]
        assert st is not None and s[0]["state"]["0"] == st, nm
        sa = s[0]["summ"][0]
        assert (sa["iterations"], sa["successful"]) == (sm["iterations"], sm["successful"]), nm
