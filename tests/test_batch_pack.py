"""The host packing stage of a batch (cerberus_amd/csrc/batch_pack.hpp) on a CPU: the HBM layout of DESIGN §3 and the guard between an
untrusted window file and the kernels' table-driven indexing.

tests/host_check/batch_pack_check.cpp reads windows written by cerberus_amd/window_io.py, optionally overwrites table entries, runs
plan_batch and fill_batch into exactly-sized heap buffers and prints every table. It is built with the undefined-behaviour sanitizer and
libstdc++'s assertions, and once more with the address sanitizer on top (that build needs to be the first library loaded: it is skipped
where the environment preloads one). `restate` below is DESIGN §3 written again in numpy, sharing nothing with the header; both must agree
exactly. tests/test_error_paths.py holds the library's status of each of the 400 table mutations against the checker's."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT
from cerberus_amd import _ctypes as T

OK, BAD_ARG, UNSUPPORTED = 0, -2, -5
MUTATION_VALUES = [-1, -7, 1 << 20, 1 << 30, 12, 97, 255, 11, 86, 87]
MUTATION_TABLES = ["lm_obs_offset", "lm_start_frame", "block_idx", "block_size", "block_id"]
POSE, SB, LB, EX, TD = range(5)   # block kinds of a prior (id = kind * 16 + index)


# ---- the checker ----
def build_checker(out_dir, asan=False):
    out = os.path.join(str(out_dir), "batch_pack_check" + ("_asan" if asan else ""))
    src = os.path.join(ROOT, "tests", "host_check", "batch_pack_check.cpp")
    san = ["-fsanitize=undefined", "-fno-sanitize-recover", "-D_GLIBCXX_ASSERTIONS"] + (["-fsanitize=address"] if asan else [])
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-pthread"] + san + [src, "-o", out], check=True, timeout=600)
    return out


@pytest.fixture(scope="module", params=["ubsan", "ubsan+asan"])
def exe(request, tmp_path_factory):
    asan = request.param == "ubsan+asan"
    if asan and os.environ.get("LD_PRELOAD"):
        pytest.skip("the address sanitizer must be the first library loaded and LD_PRELOAD is set (%s): only the build without it runs" % os.environ["LD_PRELOAD"])
    return build_checker(tmp_path_factory.mktemp("batch_pack"), asan)


def run_checker(exe, files, mutations=(), env=None):
    """mutations: (window, table, index, value). Returns (status, message, tables); a sanitizer report fails the call."""
    e = {k: v for k, v in os.environ.items() if not k.startswith("VILO_")}
    e.update(env or {})
    args = [exe]
    for m in mutations:
        args += ["--mutate"] + [str(v) for v in m]
    p = subprocess.run(args + list(files), env=e, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0 and p.stderr == "", (mutations, p.returncode, p.stderr[-2000:])
    lines = p.stdout.split("\n")
    status, message = int(lines[0].split()[1]), lines[1][len("message "):]
    tables = {}
    for ln in lines[2:]:
        if ln:
            name, _, rest = ln.partition(" ")
            tables[name] = np.array(rest.split(), dtype=np.float64 if name in FLOAT_TABLES or name[:3] in ("J0_", "r0_") else np.int64)
    return status, message, tables


FLOAT_TABLES = {"lam0", "obs", "x0", "prior_x0"}


def table_mutations(L, n_blocks):
    """The 400 single-entry mutations of tests/test_error_paths.py (generator, seed and values are that test's): (table, index, value)."""
    rng = np.random.default_rng(11)
    out = []
    for k in range(400):
        what = k % 5
        big = int(rng.choice(MUTATION_VALUES))
        hi = (L + 1, L, n_blocks, n_blocks, n_blocks)[what]
        out.append((MUTATION_TABLES[what], int(rng.integers(0, hi)), big))
    return out


def mutation_window(cfg, ocfg):
    from cerberus_amd import synth
    from oracle import oracle_py as O
    w = synth.make_window(cfg, n_landmarks=30, seed=77)
    O.fill_preint(ocfg, w)
    return w


def checker_statuses(exe, cfg, w, path):
    """The packer's status (and message) of each table mutation of window w, written to `path`."""
    from cerberus_amd import window_io
    window_io.save(path, cfg, w)
    return [run_checker(exe, [path], [(0,) + m])[:2] for m in table_mutations(w.L, w.prior.struct.n_blocks)]


# ---- windows of any shape ----
def make_window(rng, F, start_frames, use_leg=1, blocks=None, td_const=1, leg_bias_const=0, ex_const=0, long_interval=None, n_obs_each=None):
    """A window of F frames with one landmark per entry of start_frames (1 .. F - start observations each), random numbers everywhere a
    number is only copied. blocks: [(kind, index)] of the prior (None: no prior)."""
    from cerberus_amd import synth
    start_frames = np.asarray(start_frames, np.int32)
    L = len(start_frames)
    K = np.array([n_obs_each or rng.integers(1, F - s + 1) for s in start_frames], np.int64)
    w = synth.Window(L, int(K.sum()), 0)
    w.F = F
    w.lm_start_frame[:] = start_frames
    w.lm_obs_offset[1:] = np.cumsum(K)
    w.obs[:] = rng.normal(size=w.obs.shape)
    w.obs_is_stereo[:] = rng.integers(0, 2, w.n_obs)
    w.pose, w.speed_bias, w.leg_bias = rng.normal(size=(F, 7)), rng.normal(size=(F, 9)), rng.normal(size=(F, 4))
    w.ex_pose, w.td, w.inv_depth = rng.normal(size=(2, 7)), rng.normal(size=1), rng.uniform(0.1, 2.0, L)
    w.use_leg, w.td_const, w.leg_bias_const, w.ex_const = use_leg, td_const, leg_bias_const, ex_const
    w.preint, w.preint_imu = rng.normal(size=(F - 1, T.PREINT_DOUBLES)), rng.normal(size=(F - 1, T.PREINT_IMU_DOUBLES))
    w.preint[:, 0] = w.preint_imu[:, 0] = 0.1
    if long_interval is not None and long_interval < F - 1:
        w.preint[long_interval, 0] = w.preint_imu[long_interval, 0] = 10.5    # no IMU factor on an interval above 10 s
    w.prior.struct.valid = 0
    if blocks is not None:
        p = w.prior.struct
        size = {POSE: 7, SB: 9, LB: 4, EX: 7, TD: 1}
        p.n_blocks, idx = len(blocks), 0
        for k, (kind, index) in enumerate(blocks):
            p.block_id[k], p.block_size[k], p.block_idx[k] = kind * 16 + index, size[kind], idx
            idx += 6 if size[kind] == 7 else size[kind]
        p.n, p.valid = idx, 1
        w.prior.x0[:], w.prior.J0[:], w.prior.r0[:] = rng.normal(size=w.prior.x0.shape), rng.normal(size=w.prior.J0.shape), rng.normal(size=w.prior.r0.shape)
    return w


def usual_prior(F, bias_frame=0):
    return [(POSE, k) for k in range(F - 1)] + [(SB, bias_frame), (LB, bias_frame), (EX, 0), (EX, 1), (TD, 0)]


def save_all(tmp_path, cfg, windows):
    from cerberus_amd import window_io
    paths = []
    for i, w in enumerate(windows):
        paths.append(str(tmp_path / ("w%d.bin" % i)))
        window_io.save(paths[-1], cfg, w)
    return paths


# ---- DESIGN §3, restated ----
STATE_OFF = {POSE: (0, 7), SB: (77, 9), LB: (176, 4), EX: (220, 7), TD: (234, 0)}          # first double of index 0, step per index
CAMERA_DIM = {POSE: (0, 6), SB: (80, 13), LB: (89, 13), EX: (66, 6), TD: (78, 0)}          # P part 0..79, B part 80 + 13 k + c (rho: c = 9..12)


def restate(windows, wave_order=1, compact_rows=1):
    r = {k: [] for k in ("wins", "chunks", "waves", "perm", "lm_s", "obs_row", "lm_off", "L", "lam0", "obs", "flags", "x0", "imu_skip", "prior_map",
                         "prior_bsize", "prior_bidx", "prior_bxoff", "prior_bstate", "prior_x0")}
    lm_total = gram_total = obs_total = flags_total = obs_rows = 0
    chunks, waves, any_prior, compact = [], [], 0, compact_rows
    for wi, w in enumerate(windows):
        F, L = w.F, w.L
        K = np.diff(w.lm_obs_offset)
        perm = np.argsort(w.lm_start_frame, kind="stable")          # grouped by start frame, list order kept inside a group
        chunk_off, wave_off, gram_off = len(chunks), len(waves), gram_total
        for s in range(F):                                           # chunks: one start frame, at most 64 landmarks
            pos = np.nonzero(w.lm_start_frame[perm] == s)[0]
            for c0 in range(0, len(pos), 64):
                part = pos[c0:c0 + 64]
                kmax = int(K[perm[part]].max())
                chunks.append(dict(win=wi, s=s, n=len(part), kmax=kmax, lm_off=lm_total + int(part[0]), lm_local=int(part[0]), gram_off=gram_total))
                gram_total += kmax
        c = chunk_off
        while c < len(chunks):                                       # waves: at most 4 chunks side by side at 8-lane boundaries, at most 64 lanes
            segs, lanes = [], 0
            while c < len(chunks) and len(segs) < 4 and lanes + -(-chunks[c]["n"] // 8) * 8 <= 64:
                segs.append((c, lanes))
                lanes += -(-chunks[c]["n"] // 8) * 8
                c += 1
            kmax = max(chunks[ci]["kmax"] for ci, _ in segs)
            image, flags = np.zeros((kmax, 11, lanes)), np.zeros((kmax, lanes), np.int64)
            for ci, lane0 in segs:
                ch = chunks[ci]
                for i in range(ch["n"]):
                    l = perm[ch["lm_local"] + i]
                    o0 = w.lm_obs_offset[l]
                    image[:K[l], :, lane0 + i] = w.obs[o0:o0 + K[l]]
                    flags[:K[l], lane0 + i] = 1 + 2 * (w.obs_is_stereo[o0:o0 + K[l]] != 0)
            waves.append(dict(win=wi, segs=segs, lanes=lanes, kmax=kmax, obs_off=obs_total, flag_off=flags_total))
            obs_total += image.size
            flags_total += flags.size
            r["obs"].append(image.ravel()); r["flags"].append(flags.ravel())
        x = np.zeros(240)                                            # vector2double order; an absent frame holds the unit quaternion
        x[0:7 * F], x[77:77 + 9 * F], x[176:176 + 4 * F] = w.pose.ravel(), w.speed_bias.ravel(), w.leg_bias.ravel()
        x[7 * np.arange(F, 11) + 6] = 1.0
        x[220:234], x[234] = w.ex_pose.ravel(), w.td[0]
        sum_dt = (w.preint if w.use_leg else w.preint_imu)[:, 0]
        r["imu_skip"].append([0 if (k + 1 < F and not sum_dt[k] > 10.0) else 1 for k in range(10)])
        pmap, tabs, px0, prior_n, prior_nb, pad = np.zeros(96, np.int64), np.zeros((4, 40), np.int64), np.zeros(280), 0, 0, -1
        p = w.prior.struct
        if p.valid and p.n > 0:
            any_prior, prior_n, prior_nb, xo = 1, p.n, p.n_blocks, 0
            for k in range(p.n_blocks):
                kind, index, size, idx = p.block_id[k] // 16, p.block_id[k] % 16, p.block_size[k], p.block_idx[k]
                tabs[:, k] = size, idx, xo, STATE_OFF[kind][0] + STATE_OFF[kind][1] * index
                local = 6 if size == 7 else size
                pmap[idx:idx + local] = CAMERA_DIM[kind][0] + CAMERA_DIM[kind][1] * index + np.arange(local)
                px0[xo:xo + size] = w.prior.x0[xo:xo + size]
                xo += size
                if kind in (SB, LB):
                    pad = index
        const_mask = (1 if (w.leg_bias_const or not w.use_leg) else 0) | (2 if w.ex_const else 0) | (4 if w.td_const else 0)
        if not w.td_const:
            compact = 0
        r["wins"].append([F, L, len(chunks) - chunk_off, w.use_leg, lm_total, chunk_off, const_mask, prior_n, gram_off, gram_total - gram_off, prior_nb, pad,
                          wave_off, len(waves) - wave_off])
        r["perm"].append(perm); r["lm_s"].append(w.lm_start_frame[perm]); r["lam0"].append(w.inv_depth[perm])
        r["obs_row"].append(obs_rows + w.lm_obs_offset[:-1][perm]); r["lm_off"].append([lm_total]); r["L"].append([L])
        r["x0"].append(x); r["prior_map"].append(pmap); r["prior_x0"].append(px0)
        for name, row in zip(("prior_bsize", "prior_bidx", "prior_bxoff", "prior_bstate"), tabs):
            r[name].append(row)
        r["J0_%d" % wi], r["r0_%d" % wi] = [w.prior.J0[:prior_n * prior_n]], [w.prior.r0[:prior_n]]
        lm_total += L
        obs_rows += int(w.lm_obs_offset[-1]) if L else 0
    r["chunks"] = [[c[k] for k in ("win", "s", "n", "kmax", "lm_off", "lm_local", "gram_off")] for c in chunks]
    for v in waves:
        seg = v["segs"] + [(0, 0)] * (4 - len(v["segs"]))
        r["waves"].append([v["win"], len(v["segs"]), v["lanes"], v["kmax"]] + [s[0] for s in seg] + [s[1] for s in seg] + [v["obs_off"], v["flag_off"]])
    order = list(range(len(waves)))
    if wave_order >= 1:
        order.sort(key=lambda i: -waves[i]["kmax"])                  # longest first (list.sort is stable)
    if wave_order == 2:                                              # groups of equal length, every group of more than 8 rotated by its number mod 8
        out, g0, gi = [], 0, 0
        while g0 < len(order):
            g1 = g0
            while g1 < len(order) and waves[order[g1]]["kmax"] == waves[order[g0]]["kmax"]:
                g1 += 1
            grp = order[g0:g1]
            rot = gi % 8 if len(grp) > 8 else 0
            out += grp[rot:] + grp[:rot]
            g0, gi = g1, gi + 1
        order = out
    r["wave_order"] = [order]
    r["totals"] = [[lm_total, gram_total, obs_total, flags_total, obs_rows, any_prior, compact, len(chunks), len(waves)]]
    return {k: (np.concatenate([np.ravel(a) for a in v]) if len(v) else np.zeros(0)) for k, v in r.items()}


def check_layout(exe, cfg, tmp_path, windows, env=None, wave_order=1, compact_rows=1):
    status, message, got = run_checker(exe, save_all(tmp_path, cfg, windows), env=env)
    assert status == OK, message
    want = restate(windows, wave_order, compact_rows)
    assert set(got) == set(want)
    for name in want:
        assert got[name].shape == want[name].shape, (name, got[name].shape, want[name].shape)
        np.testing.assert_array_equal(got[name], want[name], err_msg=name)
    return got


@pytest.mark.parametrize("L", [0, 1, 64, 65, 600])
def test_landmark_counts(exe, cfg, tmp_path, L):
    rng = np.random.default_rng(100 + L)
    check_layout(exe, cfg, tmp_path, [make_window(rng, 11, rng.integers(0, 10, L), blocks=usual_prior(11), long_interval=3)])


@pytest.mark.parametrize("L,s", [(1, 0), (64, 3), (65, 9), (130, 2), (600, 0)])
def test_all_landmarks_on_one_start_frame(exe, cfg, tmp_path, L, s):
    rng = np.random.default_rng(200 + L)
    got = check_layout(exe, cfg, tmp_path, [make_window(rng, 11, np.full(L, s), blocks=None)])
    assert got["totals"][7] == -(-L // 64)    # chunks of at most 64


@pytest.mark.parametrize("F", range(2, 12))
@pytest.mark.parametrize("use_leg", [0, 1])
def test_window_lengths_and_factor_kinds(exe, cfg, tmp_path, F, use_leg):
    rng = np.random.default_rng(300 + 2 * F + use_leg)
    blocks = usual_prior(F, bias_frame=F - 2) if F % 2 else None
    check_layout(exe, cfg, tmp_path, [make_window(rng, F, rng.integers(0, F - 1, 20), use_leg=use_leg, blocks=blocks, leg_bias_const=F % 3 == 0,
                                                  ex_const=F % 4 == 0, long_interval=F - 3 if F > 4 else None)])


def mixed_batch(rng):
    return [make_window(rng, 11, rng.integers(0, 10, 150), blocks=usual_prior(11)), make_window(rng, 4, rng.integers(0, 3, 7)),
            make_window(rng, 11, [], blocks=usual_prior(11, 1)), make_window(rng, 7, np.full(70, 1), blocks=usual_prior(7)),
            make_window(rng, 11, rng.integers(0, 10, 600)), make_window(rng, 2, [0, 0, 0]), make_window(rng, 9, rng.integers(0, 8, 65), blocks=[(TD, 0), (EX, 1)])]


def test_a_batch_mixing_sizes(exe, cfg, tmp_path):
    check_layout(exe, cfg, tmp_path, mixed_batch(np.random.default_rng(400)))


@pytest.mark.parametrize("order", [None, 0, 1, 2])
def test_wave_order(exe, cfg, tmp_path, order):
    env = {} if order is None else {"VILO_WAVE_ORDER": str(order)}
    rng = np.random.default_rng(401)
    ws = mixed_batch(rng) + [make_window(rng, 11, np.full(600, 0), n_obs_each=11), make_window(rng, 11, np.full(600, 1), n_obs_each=10)]
    got = check_layout(exe, cfg, tmp_path, ws, env=env, wave_order=1 if order is None else order)
    kmax = got["waves"].reshape(-1, 14)[:, 3]
    assert np.bincount(kmax)[10] > 8 and np.bincount(kmax)[11] > 8    # (groups the rotated order turns: the second one by one place)


def test_compact_flag(exe, cfg, tmp_path):
    """Compact rows: td a constant block in every window of the batch, and the context allows them."""
    rng = np.random.default_rng(402)
    ws = [make_window(rng, 11, rng.integers(0, 10, 30)), make_window(rng, 11, rng.integers(0, 10, 30))]
    assert check_layout(exe, cfg, tmp_path, ws)["totals"][6] == 1
    assert check_layout(exe, cfg, tmp_path, ws, env={"CHECK_COMPACT_ROWS": "0"}, compact_rows=0)["totals"][6] == 0
    ws[1].td_const = 0
    assert check_layout(exe, cfg, tmp_path, ws)["totals"][6] == 0


# ---- untrusted tables ----
def test_mutated_tables_are_refused_before_packing(exe, cfg, ocfg, tmp_path):
    """The 400 seeded single-entry mutations of tests/test_error_paths.py: every run ends with OK, BAD_ARG or UNSUPPORTED, a refusal
    carries a message, no sanitizer reports (run_checker), and most mutations are refused: any entry set to -1, -7, 2^20, 2^30, 255, 97,
    86 or 87 (8 of the 10 values) is out of every table's range."""
    w = mutation_window(cfg, ocfg)
    outcomes = {OK: 0, BAD_ARG: 0, UNSUPPORTED: 0}
    for k, (status, message) in enumerate(checker_statuses(exe, cfg, w, str(tmp_path / "w.bin"))):
        assert status in outcomes, (k, status)
        outcomes[status] += 1
        if status != OK:
            assert len(message) > 0, k
    print("mutated tables:", outcomes)
    assert outcomes[BAD_ARG] + outcomes[UNSUPPORTED] > 300, outcomes


def test_named_messages(exe, cfg, tmp_path):
    rng = np.random.default_rng(500)
    F = 11
    ws = [make_window(rng, F, np.arange(12) % 3, blocks=usual_prior(F), n_obs_each=2) for _ in range(2)]   # blocks: poses 0 .. 9, SB 0, LB 0, EX 0, EX 1, TD
    paths = save_all(tmp_path, cfg, ws)

    def refuse(*mutations):
        status, message, _ = run_checker(exe, paths, mutations)
        return status, message

    assert refuse() == (OK, "")
    status, message = refuse((0, "lm_start_frame", 3, 11))                   # start frame outside the 11-frame window
    assert status == BAD_ARG and message.startswith("landmark observation table:")
    assert refuse((0, "lm_start_frame", 3, 10)) == (BAD_ARG, "landmark observation range outside the window")   # its two observations no longer fit
    assert refuse((0, "n_frames", 0, 12)) == (BAD_ARG, "window sizes out of range")
    status, message = refuse((1, "use_leg", 0, 0))
    assert status == UNSUPPORTED and "use_leg" in message
    assert refuse((0, "block_id", 0, 5 * 16 + 3)) == (UNSUPPORTED, "unsupported prior block")            # a feature block: not camera-side
    assert refuse((0, "block_idx", 2, 6)) == (UNSUPPORTED, "unsupported prior block")                    # overlaps block 1
    assert refuse((0, "block_id", 11, SB * 16)) == (BAD_ARG, "prior block table out of range")           # (block 11 has the leg bias's 4 doubles)
    assert refuse((0, "block_id", 11, LB * 16 + 4)) == (UNSUPPORTED, "prior couples speed/leg biases of two frames")
    assert refuse((0, "block_idx", 5, 96)) == (BAD_ARG, "prior block table out of range")
    # precedence: the lowest window among defects of the table pass ...
    assert refuse((1, "n_frames", 0, 12), (0, "lm_start_frame", 3, 10))[1] == "landmark observation range outside the window"
    assert refuse((0, "block_idx", 5, 96), (1, "lm_start_frame", 3, 11))[1] == "prior block table out of range"
    # ... any of them before an unsupported prior of whatever window ...
    assert refuse((0, "block_id", 0, 5 * 16 + 3), (1, "lm_start_frame", 3, 10)) == (BAD_ARG, "landmark observation range outside the window")
    assert refuse((0, "block_id", 11, LB * 16 + 4), (1, "block_idx", 5, 96)) == (BAD_ARG, "prior block table out of range")
    # ... and the lowest window among unsupported priors
    assert refuse((0, "block_id", 11, LB * 16 + 4), (1, "block_id", 0, 5 * 16 + 3))[1] == "prior couples speed/leg biases of two frames"
    assert refuse((1, "block_id", 11, LB * 16 + 4), (0, "block_id", 0, 5 * 16 + 3))[1] == "unsupported prior block"
    # inside one prior the first defective block decides
    assert refuse((0, "block_id", 11, LB * 16 + 4), (0, "block_id", 12, 5 * 16))[1] == "prior couples speed/leg biases of two frames"
