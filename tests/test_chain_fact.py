"""The three-stage solver factorises the bias chain four windows per wave (k_chain_fact: one window per 16-lane group) ahead of the T
recurrence (k_chain). Entry by entry the arithmetic is the single-wave solver's, so everything is held BITWISE: against the `wave` form
in this process and against the one-kernel chain (k_chain_single behind VILO_CHAIN_SINGLE, read once per process: one subprocess for all
cases) — states, cost and radius traces, summaries, retry counts and the hand-over buffers M_k, T_A(k) (also against `wave`, which
writes them too) and T(k) through vilo_debug_fetch.
  - 1, 3, 4, 5 and 9 windows: partial and full groups of four, a last wave of one; generator, field (8 frames beside 11, no prior) and
    constant-mask windows next to each other, so the four lane groups of a wave differ in frame count, mask and prior;
  - eight equal windows give equal bits at every position of the two waves;
  - a window whose factorisation fails at the initial mu sits in each of the four groups in turn beside three healthy windows: it retries
    and ends as in the `wave` form, and the neighbours end as they do in a batch without it;
  - far-off starts whose steps are rejected (the linearisation kept: the group does nothing that iteration) share a wave with plain windows;
  - the 2049-window batch of tests/frame_windows.py: every frame count from 2 to 11, four different ones in every wave, 2 frames beside 11
    and 10 (a shorter window joins the wave's walk over the shared largest frame count at its own top frame).
Four iterations each (twelve for the rejected steps, as tests/test_solver_forms.py needs them), with mu changing between them."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FIELDS = ("state", "cost", "radius", "summary", "retries")


@pytest.fixture(scope="module")
def results(tmp_path_factory):
    import _chain_fact_worker as CF
    out = str(tmp_path_factory.mktemp("chain_fact") / "single.npz")
    env = dict(os.environ, VILO_CHAIN_SINGLE="1")
    env.pop("VILO_SOLVER", None)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_chain_fact_worker.py"), out], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0 and "CHAIN_FACT_WORKER_DONE" in p.stdout, p.stderr[-2000:]
    assert "VILO_CHAIN_SINGLE" not in os.environ   # (this process runs the default: k_chain_fact + k_chain)
    with np.load(out) as z:
        single = {k: z[k] for k in z.files}
    return {"fact": CF.solve_all("split"), "wave": CF.solve_all("wave"), "single": single}


def test_the_two_processes_ran_different_chain_forms(results):
    """Without this, `fact == single` would hold trivially if the switch stopped being honoured or the default fell back to the one kernel:
    per-kernel launch counts of one four-iteration solve in each process (k_chain's row counts whichever chain kernel the plan names)."""
    fact, wave, single = results["fact"], results["wave"], results["single"]
    assert fact["launches/k_chain_fact"][0] == 4 and fact["launches/k_chain"][0] == 4
    assert single["launches/k_chain_fact"][0] == 0 and single["launches/k_chain"][0] == 4
    assert wave["launches/k_chain_fact"][0] == 0 and wave["launches/k_chain"][0] == 0


def _same(a, b, key):
    assert a[key].shape == b[key].shape and a[key].tobytes() == b[key].tobytes(), key


def _windows(res, case):
    n = 0
    while "%s/%d/state" % (case, n) in res:
        n += 1
    return n


def _check_case(results, case, keep=None):
    fact, wave, single = results["fact"], results["wave"], results["single"]
    n = _windows(fact, case) if keep is None else len(keep)
    assert n > 0 and (keep is not None or n == _windows(wave, case) == _windows(single, case))
    if keep is not None:   # the three forms kept the same windows
        key = lambda res: sorted(k for k in res if k.startswith(case + "/") and k.endswith("/state"))   # noqa: E731
        assert key(fact) == key(wave) == key(single) == sorted("%s/%d/state" % (case, i) for i in keep)
    for i in (range(n) if keep is None else keep):
        for f in FIELDS:
            _same(fact, wave, "%s/%d/%s" % (case, i, f))
            _same(fact, single, "%s/%d/%s" % (case, i, f))
        for f in ("M", "TA"):
            _same(fact, wave, "%s/%d/%s" % (case, i, f))
            _same(fact, single, "%s/%d/%s" % (case, i, f))
        if fact["%s/%d/retries" % (case, i)][0] == 0:   # (a window that went through the complete path: its T(k) is whatever the chain left)
            _same(fact, single, "%s/%d/T" % (case, i))
    return n


@pytest.mark.parametrize("W", [1, 3, 4, 5, 9])
def test_mixed_windows_in_partial_and_full_groups(results, W):
    import _chain_fact_worker as CF
    assert _check_case(results, "mixed%d" % W) == W
    # the same window at the same position of a smaller batch: the neighbours of a group do not reach it
    for i in range(min(W, 3)):
        for f in FIELDS + ("M", "TA", "T"):
            assert results["fact"]["mixed%d/%d/%s" % (W, i, f)].tobytes() == results["fact"]["mixed9/%d/%s" % (i, f)].tobytes(), (i, f)
    assert CF.MIXED[2] == "f60_partial8" and results["fact"]["mixed9/2/M"].size == 8 * 169 and results["fact"]["mixed9/0/M"].size == 11 * 169


def test_equal_windows_give_equal_bits_at_every_position(results):
    assert _check_case(results, "equal8") == 8
    for i in range(1, 8):
        for f in FIELDS + ("M", "TA", "T"):
            assert results["fact"]["equal8/%d/%s" % (i, f)].tobytes() == results["fact"]["equal8/0/%s" % f].tobytes(), (i, f)


@pytest.mark.parametrize("pos", [0, 1, 2, 3])
def test_a_failing_factorisation_leaves_its_neighbours_alone(results, pos):
    case = "fail_at%d" % pos
    assert _check_case(results, case) == 4 and _check_case(results, "healthy3") == 3
    fact = results["fact"]
    assert fact["%s/%d/retries" % (case, pos)][0] >= 1
    others = [i for i in range(4) if i != pos]
    for j, i in enumerate(others):
        assert fact["%s/%d/retries" % (case, i)][0] == 0
        for f in FIELDS + ("M", "TA", "T"):
            assert fact["%s/%d/%s" % (case, i, f)].tobytes() == fact["healthy3/%d/%s" % (j, f)].tobytes(), (i, f)
    for f in FIELDS:   # the failing window itself: the same answer in whichever group it sits
        assert fact["%s/%d/%s" % (case, pos, f)].tobytes() == fact["fail_at0/0/%s" % f].tobytes(), f


def test_rejected_steps_beside_fresh_linearisations_in_one_wave(results):
    assert _check_case(results, "rejected") == 4
    s = [results["fact"]["rejected/%d/summary" % i] for i in range(4)]
    assert all(s[i][1] + 2 <= s[i][0] for i in (1, 3))   # (rejected steps happened in the far-off windows)


def test_every_frame_count_in_waves_of_four_different_ones(results):
    """The frames batch at 2049 windows: the split form against the one-kernel chain and the `wave` form, bitwise in states, summaries and
    the hand-over buffers under tk_written's mask, at the first 32 positions, the last 33 and each window's first, middle and last one;
    and one window, one answer wherever it sits."""
    import _chain_fact_worker as CF
    import frame_windows as FR
    case = "frames%d" % CF.FRAMES_W
    keep = CF.KEEP[case]
    assert len(keep) >= 65 and keep[:4] == [0, 1, 2, 3] and keep[-1] == CF.FRAMES_W - 1
    assert _check_case(results, case, keep) == len(keep)
    fact = results["fact"]
    frames = {nm: rec[0] for nm, rec in FR.LEG.items()}
    seen = {}
    for i in keep:
        nm = FR.LEG_ORDER[i % len(FR.LEG_ORDER)]
        assert fact["%s/%d/M" % (case, i)].size == 169 * frames[nm] and fact["%s/%d/retries" % (case, i)][0] == 0, (i, nm)
        first = seen.setdefault(nm, i)
        for f in FIELDS + ("M", "TA", "T"):
            assert fact["%s/%d/%s" % (case, i, f)].tobytes() == fact["%s/%d/%s" % (case, first, f)].tobytes(), (i, nm, f)
    assert set(seen) == set(FR.LEG) and sorted(set(frames.values())) == list(range(2, 12))
    assert [frames[FR.LEG_ORDER[i]] for i in range(4)] == [2, 11, 3, 10] and [frames[FR.LEG_ORDER[i]] for i in range(16, 20)] == [10, 2, 9, 3]
