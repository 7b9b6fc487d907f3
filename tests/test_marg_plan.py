"""The host bookkeeping of a marginalisation call (cerberus_amd/csrc/marg_plan.hpp) on a CPU: which blocks a window's marginalisation
drops and keeps, the cdmap the kernels build A and b through, the dropped-landmark list, and the kept-block table and x0 of the prior that
comes out — what replaces the reference's address-keyed addr_shift.

tests/host_check/marg_plan_check.cpp reads windows written by cerberus_amd/window_io.py, runs plan_batch for the landmark order, then
plan_marginalization, assign_marg_scratch and the two write-out functions into exactly-sized heap buffers, and prints every table. It is
built with the undefined-behaviour sanitizer and libstdc++'s assertions, and once more with the address sanitizer on top (that build needs
to be the first library loaded: it is skipped where the environment preloads one). The oracle's marginalisation of the same window and
mode (oracle_py.marginalize) gives the prior's blocks, n, valid, x0 and the dropped dimension m; they must agree exactly."""
import functools
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

OK, UNSUPPORTED = 0, -5
POSE, SB, LB, EX, TD = range(5)
CD_N = 224
LOCAL = {POSE: 6, SB: 9, LB: 4, EX: 6, TD: 1}                                             # local size of a block kind
STATE_OFF = {POSE: (0, 7), SB: (77, 9), LB: (176, 4), EX: (220, 7), TD: (234, 0)}          # first double of index 0, step per index
CAMERA_DIM = {POSE: (0, 6), SB: (80, 13), LB: (89, 13), EX: (66, 6), TD: (78, 0)}
CASES = ["prior", "no_prior", "no_leg", "long_interval0", "short", "no_frame0_landmarks", "masked"]
MAX_PRIOR_DIM, MAX_PRIOR_BLOCKS, MAX_DROPPED = 96, 40, 1200


def build_checker(out_dir, asan=False):
    out = os.path.join(str(out_dir), "marg_plan_check" + ("_asan" if asan else ""))
    src = os.path.join(ROOT, "tests", "host_check", "marg_plan_check.cpp")
    san = ["-fsanitize=undefined", "-fno-sanitize-recover", "-D_GLIBCXX_ASSERTIONS"] + (["-fsanitize=address"] if asan else [])
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + san + [src, "-o", out], check=True, timeout=600)
    return out


@pytest.fixture(scope="module", params=["ubsan", "ubsan+asan"])
def exe(request, tmp_path_factory):
    asan = request.param == "ubsan+asan"
    if asan and os.environ.get("LD_PRELOAD"):
        pytest.skip("the address sanitizer must be the first library loaded and LD_PRELOAD is set (%s): only the build without it runs" % os.environ["LD_PRELOAD"])
    return build_checker(tmp_path_factory.mktemp("marg_plan"), asan)


def run_checker(exe, files, mode, mask=(), unpacked=False):
    """(status, tables); a sanitizer report fails the call."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("VILO_")}
    args = [exe, "--mode", str(mode)] + (["--mask", ",".join(str(int(l)) for l in mask)] if len(mask) else []) + (["--unpacked"] if unpacked else [])
    p = subprocess.run(args + list(files), env=e, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (p.returncode, p.stderr[-2000:])
    lines = p.stdout.split("\n")
    tables = {}
    for ln in lines[1:]:
        if ln:
            name, _, rest = ln.partition(" ")
            tables[name] = np.array(rest.split(), dtype=np.float64 if name.startswith("x0_") else np.int64)
    return int(lines[0].split()[1]), tables


# ---- the cases: (the window the planner sees, its mask, the window the oracle sees) ----
@functools.lru_cache(maxsize=None)
def case(name):
    import mask_ref
    from _paths_worker import _truncate
    from cerberus_amd import synth
    from oracle import oracle_py as O
    cfg = synth.default_config()
    w = synth.make_window(cfg, n_landmarks=20 + 2 * CASES.index(name), seed=300 + CASES.index(name))
    O.fill_preint(O.config_from(cfg), w)
    ref = w
    if name == "no_prior":
        w.prior.struct.valid = 0
    elif name == "no_leg":
        w.use_leg = 0
    elif name == "long_interval0":
        w.preint[0, 0] = w.preint_imu[0, 0] = 10.5     # sum_dt > 10 s: no IMU factor on interval 0,
        w.prior.struct.valid = 0                       # and no prior on the speed / leg biases of frame 0 either
    elif name == "short":
        w = ref = _truncate(w, 7)                       # (no prior; the file holds the arrays of 7 frames)
        w.pose, w.speed_bias, w.leg_bias = w.pose[:7].copy(), w.speed_bias[:7].copy(), w.leg_bias[:7].copy()
        w.preint, w.preint_imu = w.preint[:6].copy(), w.preint_imu[:6].copy()
    elif name == "no_frame0_landmarks":
        w = ref = mask_ref.delete_landmarks(w, w.lm_start_frame == 0)
        assert w.L > 0
    mask = np.zeros(w.L, np.uint8)
    if name == "masked":
        frame0 = np.flatnonzero(w.lm_start_frame == 0)
        assert len(frame0) >= 4
        mask[frame0[1::2]] = 1                          # every other landmark of frame 0
        ref = mask_ref.delete_landmarks(w, mask)
    return w, mask, ref


@functools.lru_cache(maxsize=None)
def oracle(name, mode):
    """(m, n, valid, blocks, x0) of the oracle's marginalisation, computed once."""
    from cerberus_amd import synth
    from cerberus_amd.synth import PriorData
    from oracle import oracle_py as O
    ref = case(name)[2]
    p = PriorData()
    rc, m, _, _ = O.marginalize(O.config_from(synth.default_config()), ref, mode, p)
    valid = int(p.struct.valid)
    blocks = p.blocks() if valid else []
    return rc, m, (p.n if valid else 0), valid, blocks, p.x0[:sum(b[1] for b in blocks)].copy()


def plan_of(exe, tmp_path, name, mode):
    from cerberus_amd import synth, window_io
    w, mask, _ = case(name)
    path = str(tmp_path / "w.bin")
    window_io.save(path, synth.default_config(), w)
    status, t = run_checker(exe, [path], mode, mask=np.flatnonzero(mask))
    assert status == OK
    return w, mask, t


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_plan_against_the_oracle(exe, tmp_path, name, mode):
    w, mask, t = plan_of(exe, tmp_path, name, mode)
    rc, om, on, ovalid, oblocks, ox0 = oracle(name, mode)
    m, n, n_drop_lm, pmode, has_imu, prior_n, skip, keep_prior, max_l0 = t["win_0"]
    pn, pnb, pvalid = t["prior_0"]
    blocks = list(zip(t["block_id_0"].tolist(), t["block_size_0"].tolist(), t["block_idx_0"].tolist()))
    print(name, mode, "m", m, om, "n", n, on, "valid", pvalid, ovalid, "oracle rc", rc, "keep_prior", keep_prior)
    assert pmode == mode and not skip
    if keep_prior:
        # MARGIN_SECOND_NEW with nothing to marginalise: the oracle leaves its output alone, the old prior carries over unchanged
        p = w.prior
        assert mode == 1 and (m, n) == (0, 0) and om == 0
        assert (pn, pvalid) == (p.n, 1) and blocks == p.blocks()
        np.testing.assert_array_equal(t["x0_0"], p.x0[:sum(b[1] for b in blocks)])
        return
    assert (m, n, pvalid) == (om, on, ovalid)
    assert pn == on and blocks == oblocks
    np.testing.assert_array_equal(t["x0_0"], ox0)
    if name == "no_prior" and mode == 1:
        assert (m, n, pvalid) == (0, 0, 0)
    if name == "long_interval0" and mode == 0:
        assert has_imu == 0 and m - n_drop_lm == 6      # the dense dropped part is the pose alone
    if name == "no_frame0_landmarks" and mode == 0:
        assert n_drop_lm == 0
    if name == "masked" and mode == 0:
        assert n_drop_lm == int(((w.lm_start_frame == 0) & (mask == 0)).sum())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("name", CASES)
def test_plan_invariants(exe, tmp_path, name, mode):
    """cdmap is injective and covers [0, m - n_drop_lm) and [m, m + n) exactly; the dropped landmarks are those of frame 0 that are not
    masked, ascending in original index; the kept blocks tile [0, n) in ascending id at the state offsets of DESIGN §3."""
    w, mask, t = plan_of(exe, tmp_path, name, mode)
    m, n, n_drop_lm = t["win_0"][:3]
    cd = t["cdmap_0"]
    assert cd.shape == (CD_N,)
    used = cd[cd >= 0]
    assert len(set(used.tolist())) == len(used)
    assert sorted(used.tolist()) == list(range(0, m - n_drop_lm)) + list(range(m, m + n))
    perm, drop = t["perm_0"], t["drop_0"]
    assert sorted(perm.tolist()) == list(range(w.L)) and len(drop) == n_drop_lm
    orig = perm[drop] if len(drop) else np.zeros(0, np.int64)
    assert np.all(np.diff(orig) > 0)
    if mode == 0:
        assert orig.tolist() == np.flatnonzero((w.lm_start_frame == 0) & (mask == 0)).tolist()
    kept = t["kept_0"].reshape(-1, 4)
    at = 0
    for bid, idx, size, soff in kept.tolist():
        kind, index = bid // 16, bid % 16
        assert idx == at and size == {6: 7}.get(LOCAL[kind], LOCAL[kind]) and soff == STATE_OFF[kind][0] + STATE_OFF[kind][1] * index
        c0 = CAMERA_DIM[kind][0] + CAMERA_DIM[kind][1] * index
        assert cd[c0:c0 + LOCAL[kind]].tolist() == list(range(m + idx, m + idx + LOCAL[kind]))
        at += LOCAL[kind]
    assert at == n and np.all(np.diff(kept[:, 0]) > 0)
    off, total = t["scratch"][0], t["scratch"][1]
    T = m + n
    assert (off, total) == ((0, T * T + T + 3 * m * m + n * m + 3 * n * n + 2 * n + 64) if m > 0 and n > 0 else (-1, 0))


# ---- the three limits ----
def _limit_window(rng, L, blocks, n_obs_each):
    from test_batch_pack import make_window
    return make_window(rng, 11, np.zeros(L, np.int32), blocks=blocks, n_obs_each=n_obs_each)


def _status(exe, tmp_path, w, unpacked=False):
    from cerberus_amd import synth, window_io
    path = str(tmp_path / "limit.bin")
    window_io.save(path, synth.default_config(), w)
    status, t = run_checker(exe, [path], 0, unpacked=unpacked)
    return status, t


def test_more_than_96_kept_dims_is_unsupported(exe, tmp_path):
    """A prior on the speed / leg biases of frame 5 beside the IMU factor's of frame 1: poses 1 .. 10 (60), two speed-bias (18) and two
    leg-bias blocks (8), extrinsics (12), td (1) = 99 kept dims in 17 blocks, 19 + 3 dropped. Without the prior's leg-bias block: 95."""
    rng = np.random.default_rng(600)
    base = [(POSE, k) for k in range(10)] + [(SB, 5), (EX, 0), (EX, 1), (TD, 0)]
    status, t = _status(exe, tmp_path, _limit_window(rng, 3, base, 11))
    assert status == OK and t["win_0"][1] == 95 and len(t["kept_0"]) // 4 == 16
    status, _ = _status(exe, tmp_path, _limit_window(rng, 3, base + [(LB, 5)], 11))
    assert status == UNSUPPORTED


def test_more_than_1200_dropped_dims_is_unsupported(exe, tmp_path):
    """19 dense dims of frame 0 and one per landmark that starts there: 1181 landmarks pass, 1182 do not. A batch takes 1000 landmarks per
    window, so this limit is the planner's own defence: the checker is run without plan_batch."""
    rng = np.random.default_rng(601)
    status, t = _status(exe, tmp_path, _limit_window(rng, 1181, None, 2), unpacked=True)
    assert status == OK and t["win_0"][0] == MAX_DROPPED and t["win_0"][1] <= MAX_PRIOR_DIM
    status, _ = _status(exe, tmp_path, _limit_window(rng, 1182, None, 2), unpacked=True)
    assert status == UNSUPPORTED


def test_the_kept_block_limit_lies_behind_the_dim_limit():
    """More than 40 kept blocks cannot be exceeded alone: block ids are distinct, an id has 16 indices, so 41 blocks take at least the 16
    of size 1, then 25 of size 4: 116 kept dims, beyond the 96 the same test refuses first. (Tables a batch accepts name at most
    11 + 11 + 11 + 2 + 1 = 36 camera-side blocks.)"""
    sizes = sorted(s for s in LOCAL.values() for _ in range(16))
    assert sum(sizes[:MAX_PRIOR_BLOCKS + 1]) > MAX_PRIOR_DIM
