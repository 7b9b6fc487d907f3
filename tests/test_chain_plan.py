"""The chain axis of the launch plan (cerberus_amd/csrc/launch_plan.hpp) on a CPU, under sanitizers (tests/host_check/chain_plan_check.cpp):
the three-stage solver plans k_chain_fact + k_chain unless VILO_CHAIN_SINGLE pins the one-kernel chain, no other solver form has a
chain axis, and the axis is part of the plan's equality — the key a captured launch sequence is replayed under."""
import os
import subprocess

import pytest

from conftest import ROOT

SINGLE, FACT, NONE = 0, 1, -1
WAVE, SPLIT, MW8 = 0, 3, 4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("chain_plan") / "chain_plan_check")
    src = os.path.join(ROOT, "tests", "host_check", "chain_plan_check.cpp")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", src, "-o", out], check=True, timeout=300)
    return out


def _plan(exe, env_extra, W, n_waves, forced=-1, iterates=1):
    env = {k: v for k, v in os.environ.items() if not k.startswith("VILO_")}
    env.update(env_extra)
    p = subprocess.run([exe, str(W), str(n_waves), str(forced), str(iterates)], env=env, capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, (p.returncode, p.stderr)
    return tuple(int(v) for v in p.stdout.split())


def test_the_three_stage_form_plans_the_two_chain_kernels_by_default(exe):
    for W in (1025, 1280, 4096, 32768):
        assert _plan(exe, {}, W, 10 * W) == (SPLIT, FACT, 1)
    assert _plan(exe, {}, 9, 9, forced=SPLIT) == (SPLIT, FACT, 1)   # (vilo_set_solver_form: small batches reach it)


def test_the_switch_pins_the_one_kernel_chain_and_changes_the_key(exe):
    for W in (1025, 32768):
        assert _plan(exe, {"VILO_CHAIN_SINGLE": "1"}, W, 10 * W) == (SPLIT, SINGLE, 0)
    assert _plan(exe, {"VILO_CHAIN_SINGLE": "1"}, 9, 9, forced=SPLIT) == (SPLIT, SINGLE, 0)


@pytest.mark.parametrize("env", [{}, {"VILO_CHAIN_SINGLE": "1"}])
def test_no_other_solver_form_has_a_chain_axis(exe, env):
    assert _plan(exe, env, 32, 32) == (MW8, NONE, 1)
    assert _plan(exe, env, 1024, 10240) == (WAVE, NONE, 1)
    assert _plan(exe, env, 32768, 327680, forced=WAVE) == (WAVE, NONE, 1)
    assert _plan(exe, env, 32768, 327680, iterates=0) == (NONE, NONE, 1)   # (a solve without iterations launches no solver)
    # the threshold of the three-stage form moves the axis with the solver
    assert _plan(exe, dict(env, VILO_SPLIT_MIN_WINDOWS="2000"), 1280, 12800)[:2] == (WAVE, NONE)
