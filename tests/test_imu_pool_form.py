"""The full batch's IMU linearisation from the block pool: k_imu_raw stores a factor's 96-double pool (imu_blocks), k_imu_linearize stages a
pair's two pools and two record heads in LDS and every lane forms its [J | r] operands through the compile-time gather table — the helper
the fused small-batch body (imu_fused_body) uses too.

CPU: the pair kernel's staging emulated on the host (tests/host_check/imu_pool_check.cpp) against imu_leg_raw / imu_raw.
GPU: the three IMU forms (fused, a pair per wave, a factor per wave) bit for bit on the same windows; batch sizes around the pair
permutation's groups, both factor kinds, intervals without a factor, against the oracle at the bounds tests/test_kernel_paths.py holds for
the same comparison (equal iterations / successful steps, cost 1e-8, states 1e-8); the whitened block (mode 0) through
vilo_batch_marginalize against the oracle's marginalisation at the per-block bound of tests/test_gpu_parity.py::test_marginalize.

A batch holds one IMU factor kind (vilo_batch_create refuses a mix of use_leg = 1 and use_leg = 0 windows, tests/test_batch_pack.py), so a
wave never meets both gather tables: each kind gets batches of its own here."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from test_host_math import P, hc  # noqa: F401  (the host build of the raw factors)

sys.path.insert(0, os.path.join(ROOT, "tests"))
import _imu_pool_worker as WK  # noqa: E402

PAIR = {"VILO_SMALL_FUSE_MAX_WINDOWS": "0", "VILO_IMU_SINGLE_MAX_WINDOWS": "0"}
SINGLE = {"VILO_SMALL_FUSE_MAX_WINDOWS": "0"}
FUSED = {}
_cache = {}


# ---------------------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pc():
    d = os.path.join(ROOT, "tests", "host_check")
    so = os.path.join(d, "libimupoolcheck.so")
    srcs = [os.path.join(d, "imu_pool_check.cpp"), os.path.join(ROOT, "cerberus_amd", "csrc", "factors.hpp"),
            os.path.join(ROOT, "cerberus_amd", "csrc", "vilo_math.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", so, srcs[0]])
    return C.CDLL(so)


def test_lane_major_table_is_the_gather_table(pc):
    assert pc.hc_imu_lane_table_mismatches() == 0


@pytest.mark.parametrize("leg", [1, 0])
def test_pair_staging_and_shared_helper_reproduce_the_raw_factors(pc, hc, cfg, ocfg, leg):  # noqa: F811
    """Three windows' 30 factors as one batch (NF = 30: a pair's entries lie 30 doubles apart in the entry-major pools); every pair's
    operand image through the kernel's staging offsets and the shared helper equals what imu_leg_raw / imu_raw write, entry by entry
    (assert_array_equal, as tests/test_host_math.py compares the fused body's image), structural zeros included."""
    from cerberus_amd import synth
    from oracle import oracle_py as O
    ws = []
    for i in range(3):
        w = synth.make_window(cfg, n_landmarks=5, seed=40 + i)
        O.fill_preint(ocfg, w)
        ws.append(w)
    NF = 30
    pre = np.ascontiguousarray(np.concatenate([w.preint[:10] for w in ws]))
    pre_imu = np.ascontiguousarray(np.concatenate([w.preint_imu[:10] for w in ws]))
    x = np.zeros((NF, 40))
    for i, w in enumerate(ws):
        for k in range(10):
            x[10 * i + k] = np.concatenate([w.pose[k], w.speed_bias[k], w.leg_bias[k], w.pose[k + 1], w.speed_bias[k + 1], w.leg_bias[k + 1]])
    for p in range(NF // 2):
        img = np.full((2, 32, 48), np.nan)
        pc.hc_imu_pair_image(NF, p, P(pre), P(pre_imu), leg, C.c_double(9.805), P(x), P(img))
        for h in range(2):
            f = 2 * p + h
            s = x[f]
            st = [np.ascontiguousarray(a) for a in (s[0:7], s[7:16], s[16:20], s[20:27], s[27:36], s[36:40])]
            if leg:
                r = np.zeros(31); J = np.zeros((31, 38))
                hc.hc_imu_leg_raw(P(np.ascontiguousarray(pre[f])), C.c_double(9.805), *[P(a) for a in st], P(r), P(J))
                np.testing.assert_array_equal(img[h, :31, :38], J)
                np.testing.assert_array_equal(img[h, :31, 38], r)
                assert not img[h, 31].any() and not img[h, :, 39:].any()
            else:
                r = np.zeros(15); J = np.zeros((15, 30))
                hc.hc_imu_raw(P(np.ascontiguousarray(pre_imu[f])), C.c_double(9.805), P(st[0]), P(st[1]), P(st[3]), P(st[4]), P(r), P(J))
                np.testing.assert_array_equal(img[h, :15, :15], J[:, :15])
                np.testing.assert_array_equal(img[h, :15, 19:34], J[:, 15:])
                np.testing.assert_array_equal(img[h, :15, 38], r)
                assert not img[h, 15:].any() and not img[h, :15, 15:19].any() and not img[h, :15, 34:38].any() and not img[h, :, 39:].any()


def test_stand_alone_host_check_program(tmp_path):
    """The same emulation as a program of its own (random heads and states, both factor kinds): what a host sanitizer build runs."""
    exe = str(tmp_path / "imu_pool_check")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-DIMU_POOL_CHECK_MAIN", "-o", exe,
                           os.path.join(ROOT, "tests", "host_check", "imu_pool_check.cpp")])
    p = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert p.returncode == 0, p.stdout[-2000:]


# ---------------------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------------------
def _run(case, env_form, marg=False):
    """One child process per (case, form): the switches are read once per process."""
    key = (case, tuple(sorted(env_form.items())), marg)
    if key not in _cache:
        env = {k: v for k, v in os.environ.items() if not k.startswith("VILO_") or k == "VILO_GPU_LIB"}
        env.update(env_form)
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_imu_pool_worker.py"), json.dumps({"case": case, "marg": marg})],
                           cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)
        assert p.returncode == 0, (case, env_form, p.stderr[-3000:])
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("IMU_POOL_JSON ")][-1]
        _cache[key] = json.loads(line[len("IMU_POOL_JSON "):])
    return _cache[key]


_oracle = {}


def _oracle_solve(cfg, ocfg, case):
    """The oracle's solve of a case's windows, once (identical windows of different cases share one solve)."""
    from oracle import oracle_py as O
    out = []
    c = WK.CASES[case]
    for i, w in enumerate(WK.windows(cfg, ocfg, case)):
        key = (i, c["use_leg"], tuple(c["skip"].get(i, [])))
        if key not in _oracle:
            s = O.solve_window(ocfg, w, O.default_opts(True, WK.ITERS))
            _oracle[key] = (s.iterations, s.num_successful, s.final_cost, [a.copy() for a in w.state_arrays()])
        out.append(_oracle[key])
    return out


def _rel_states(a_list, b_list):
    worst = 0.0
    for a, b in zip(a_list, b_list):
        a, b = np.asarray(a, float), np.asarray(b, float)
        if a.size:
            worst = max(worst, float(np.abs(a - b).max() / max(1.0, np.abs(b).max())))
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["w7_skip", "w7_imu_skip"])
def test_the_three_imu_forms_are_bitwise_the_same(case):
    """Fused into the visual launch, k_imu_raw + k_imu_linearize with a pair per wave, the same with a factor per wave: the same windows,
    child processes that differ only in the two IMU switches. The descriptor: the IMU axis takes its three values; the visual axis names
    the same frame-parallel compact body with (small_c) and without (tpar_c) the IMU workgroups in its launch, imu_order exists only for
    the fused form; assembly, solver and rows do not move. Final states, cost traces and summaries: identical."""
    fused, pair, single = _run(case, FUSED), _run(case, PAIR), _run(case, SINGLE)
    assert (fused["path"]["imu"], pair["path"]["imu"], single["path"]["imu"]) == ("fused", "pair", "single")
    assert (fused["path"]["visual"], pair["path"]["visual"], single["path"]["visual"]) == ("small_c", "tpar_c", "tpar_c")
    assert (fused["path"]["imu_order"], pair["path"]["imu_order"], single["path"]["imu_order"]) == ("first", "none", "none")
    for ax in ("assembly", "solver", "rows", "replay", "wave_order"):
        assert fused["path"][ax] == pair["path"][ax] == single["path"][ax], ax
    for other in (pair, single):
        assert other["digest"] == fused["digest"]
        assert other["state"] == fused["state"]
        assert other["summ"] == fused["summ"]   # (iterations, decisions, final cost and the whole cost trace, as Python floats: bitwise)


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(WK.CASES))
def test_pair_form_against_the_oracle(cfg, ocfg, case):
    """W = 1 / 7 / 13 (5, 35, 65 pairs: the permutation's identity branch, one group plus a tail, two groups plus a tail), both factor
    kinds, intervals without a factor as the first, the second and both factors of a pair."""
    res = _run(case, PAIR, marg=case in ("w7_skip", "w7_imu_skip"))
    assert res["path"]["imu"] == "pair"
    worst = worst_c = 0.0
    for i, (it, ok, cost, st) in enumerate(_oracle_solve(cfg, ocfg, case)):
        sm = res["summ"][i]
        assert (sm["iterations"], sm["successful"]) == (it, ok), (case, i)
        np.testing.assert_allclose(sm["final_cost"], cost, rtol=1e-8, err_msg="%s %d" % (case, i))
        e = _rel_states(res["state"][i], st)
        worst, worst_c = max(worst, e), max(worst_c, abs(sm["final_cost"] / cost - 1))
        assert e < 1e-8, (case, i, e)
    print("MEASURED test_imu_pool_form[%s] vs oracle: states %.2e, cost %.2e" % (case, worst, worst_c))


class _Prior:
    """What tests/marg_exact.py reads of a synth.PriorData, from the worker's JSON."""

    def __init__(self, d):
        from cerberus_amd import _ctypes as T
        self.struct = T.Prior()
        self.struct.n, self.struct.n_blocks, self.struct.valid = d["n"], len(d["blocks"]), d["valid"]
        for k, (bid, size, idx) in enumerate(d["blocks"]):
            self.struct.block_id[k], self.struct.block_size[k], self.struct.block_idx[k] = bid, size, idx
        self.J0, self.r0 = np.array(d["J0"]), np.array(d["r0"])

    def blocks(self):
        return [(self.struct.block_id[k], self.struct.block_size[k], self.struct.block_idx[k]) for k in range(self.struct.n_blocks)]


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["w7_skip", "w7_imu_skip"])
def test_mode_0_whitened_block_through_the_marginalisation(cfg, ocfg, case):
    """vilo_batch_marginalize (MARGIN_OLD) of the seven windows at their solved states: its linearisation pass runs k_imu_raw +
    k_imu_linearize in mode 0, which stores the whitened [J | r] block the marginalisation reads. Against the oracle's marginalisation of
    the same states, per kept block pair in units of the blocks' own diagonals (tests/marg_exact.py), at test_marginalize's bound for
    this mode: 2e-5."""
    from cerberus_amd.synth import PriorData
    from marg_exact import block_table, exact_schur, scaled_errors
    from oracle import oracle_py as O
    res = _run(case, PAIR, marg=True)
    worst = 0.0
    for i, w in enumerate(WK.windows(cfg, ocfg, case)):
        w.set_state([np.array(a) for a in res["state"][i]])
        po = PriorData()
        rc, m, A, bvec = O.marginalize(ocfg, w, 0, po, want_A=True)
        pg = _Prior(res["prior"][i])
        assert rc == 0 and pg.struct.valid == 1 and pg.blocks() == po.blocks(), (case, i)
        He, ge = exact_schur(A, bvec, m)
        eh, eb, _, _ = scaled_errors(pg, He, ge, block_table(po))
        worst = max(worst, eh, eb)
        assert max(eh, eb) < 2e-5, (case, i, eh, eb)
    print("MEASURED test_imu_pool_form[%s] marginalisation vs exact Schur complement: %.2e of the blocks' diagonals" % (case, worst))
