"""The launch plan (cerberus_amd/csrc/launch_plan.hpp) on a CPU: which kernel forms a batch shape selects under which switches.

tests/test_kernel_paths.py pins the same table on a GPU, by launching; this one pins the pure function behind it. Every row of that test,
under the row's environment in a process of its own (the switches are read once per process), must plan the descriptor the row expects:
the W = 32 rows at 1 and at 256 packed waves (the frame-parallel form's threshold), row N's sizes at 257 packed waves and at ten per
window, few300 at 1 and at 256. Then the lane rule at its threshold edges and the shapes no row of that table has."""
import os
import subprocess

import pytest

from conftest import ROOT
from cerberus_amd._ctypes import PATH_AXES
from test_kernel_paths import EXPECT, ROWS, WAVE_ORDER

SOLVER = {"wave": 0, "split": 3, "mw8": 4}   # VILO_SOLVER: the default vilo_create gives a context's solver form (include/vilo_gpu.h)
# row M's switches (record upload, host staging) select no kernel: its plan is the default one, row A's
EXPECT_ROW = dict(EXPECT, M=EXPECT["A"])
COST = {-1: "none", 0: "tpar", 1: "walk"}


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_check")
    src = os.path.join(ROOT, "tests", "host_check", "launch_plan_check.cpp")
    subprocess.run(["g++", "-O2", "-std=c++17", src, "-o", out], check=True, timeout=300)
    return out


def _call(exe, env_row, *args):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VILO_")}
    env.update(env_row)
    p = subprocess.run([exe] + [str(a) for a in args], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (args, p.returncode, p.stderr)
    return [int(v) for v in p.stdout.split()]


def _plan(exe, env_row, W, n_waves, compact=1, full_regime=0, forced=-1, iterates=1, mode="plan"):
    args = ("marg", n_waves, full_regime) if mode == "marg" else ("plan", W, n_waves, compact, full_regime, forced, iterates)
    v = _call(exe, env_row, *args)
    d = {axis: names[c] for (axis, names), c in zip(PATH_AXES, v[:6])}
    d.update(cost=COST[v[6]], tpar=v[7], wave_order=v[8], no_graph=v[9])
    return d


@pytest.mark.parametrize("row", list(ROWS))
def test_every_row_of_the_kernel_path_table(row, exe):
    env_row, spec = ROWS[row]
    compact = 0 if (spec.get("compact", 1) == 0 or spec.get("td")) else 1   # (a window that estimates td: 23 columns for the batch)
    forced = SOLVER.get(env_row.get("VILO_SOLVER"), -1)
    cases = [(str(W) if row == "N" else row, W, nw) for W in spec.get("sizes", [32]) for nw in ((257, 10 * W) if row == "N" else (1, 256))]
    cases += [("few%d" % W, W, nw) for W in spec.get("few_sizes", []) for nw in (1, 256)]
    for name, W, n_waves in cases:
        assert name in EXPECT_ROW, "no expectation stated for %s" % name
        got = _plan(exe, env_row, W, n_waves, compact=compact, forced=forced)
        assert {k: got[k] for k in EXPECT_ROW[name]} == EXPECT_ROW[name], (row, name, n_waves, got)
        assert got["wave_order"] == WAVE_ORDER.get(row, 1), (row, got)
        assert got["no_graph"] == (1 if row == "L" else 0), (row, got)
        assert got["cost"] == ("tpar" if got["tpar"] else "walk"), (row, got)


def _p(visual, imu, imu_order, assembly, solver, rows, cost):
    return dict(visual=visual, imu=imu, imu_order=imu_order, assembly=assembly, solver=solver, rows=rows, cost=cost)


def _axes(got):
    return {k: got[k] for k in ("visual", "imu", "imu_order", "assembly", "solver", "rows", "cost")}


def test_lane_rule_at_the_threshold_edges(exe):
    """A call is cut into lanes only if as one batch it would be a full one: more than 256 windows (small assembly) and more than 256
    windows with landmarks (each at least one packed wave: frame-parallel form)."""
    assert _call(exe, {}, "lanes", 256, 256) == [0]
    assert _call(exe, {}, "lanes", 257, 257) == [1]
    assert _call(exe, {}, "lanes", 256, 4096) == [0]
    assert _call(exe, {}, "lanes", 257, 4096) == [1]
    assert _call(exe, {}, "lanes", 4096, 256) == [0]
    assert _call(exe, {}, "lanes", 4096, 257) == [1]
    # the thresholds are the plan's own: moved switches move the rule
    assert _call(exe, {"VILO_ASM_SMALL_MAX_WINDOWS": "0", "VILO_NO_TPAR": "1"}, "lanes", 1, 1) == [1]


def test_full_regime_takes_the_full_kernel_set_at_any_size(exe):
    """A lane's share of 7 windows and 3 packed waves: no small assembly, no frame-parallel form; what a full batch of up to 256 windows runs."""
    got = _plan(exe, {}, 7, 3, full_regime=1)
    assert got["tpar"] == 0
    assert _axes(got) == _p("pc_imu", "fused", "first", "full", "mw8", "compact", "walk")
    # the same shape as a batch of its own is a small one
    got = _plan(exe, {}, 7, 3)
    assert got["tpar"] == 1
    assert _axes(got) == _p("small_c", "fused", "first", "small", "mw8", "compact", "tpar")


@pytest.mark.parametrize("W,forced,solver", [(32, 0, "wave"), (32, 3, "split"), (4096, 4, "mw8"), (4096, 0, "wave"),
                                             (512, -1, "mw8"), (513, -1, "wave"), (1024, -1, "wave"), (1025, -1, "split")])
def test_forced_solver_form_overrides_size(exe, W, forced, solver):
    assert _plan(exe, {}, W, 10 * W, forced=forced)["solver"] == solver


def test_no_packed_waves(exe):
    """No landmark in the batch: no visual launch, no visual cost, the IMU factors in kernels of their own."""
    assert _axes(_plan(exe, {}, 32, 0)) == _p("none", "single", "none", "small", "mw8", "compact", "none")
    assert _axes(_plan(exe, {}, 300, 0)) == _p("none", "pair", "none", "full", "mw8", "compact", "none")
    assert _axes(_plan(exe, {}, 32, 0, compact=0)) == _p("none", "single", "none", "accept_wave", "mw8", "full", "none")


def test_no_iterations(exe):
    """max_num_iterations = 0: only the costs are launched; every axis but the rows reads none."""
    assert _axes(_plan(exe, {}, 32, 40, iterates=0)) == _p("none", "none", "none", "none", "none", "compact", "tpar")
    assert _axes(_plan(exe, {}, 4096, 40960, compact=0, iterates=0)) == _p("none", "none", "none", "none", "none", "full", "walk")


def test_marginalisation_pass(exe):
    """vilo_marg_linearize: 23-column rows, frame-parallel or not as the batch was created, the IMU factors unfused, a pair per wave."""
    assert _axes(_plan(exe, {}, 0, 10, mode="marg")) == _p("tpar", "pair", "none", "none", "none", "full", "none")
    assert _axes(_plan(exe, {}, 0, 300, mode="marg")) == _p("single", "pair", "none", "none", "none", "full", "none")
    assert _axes(_plan(exe, {}, 0, 10, full_regime=1, mode="marg")) == _p("single", "pair", "none", "none", "none", "full", "none")
    assert _axes(_plan(exe, {}, 0, 0, mode="marg")) == _p("none", "pair", "none", "none", "none", "full", "none")
