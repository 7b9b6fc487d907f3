"""Worker of test_kernel_paths.py: solves a fixed window set through a resident batch under the tuning switches the environment pins (the
library reads them once per process) and prints, as JSON, the descriptor of every solve (vilo_debug_batch_path), a digest of every
window's final state, every window's summary and the full states of the special windows.

Spec key "field": a further resident batch (32 windows, or spec["field_sizes"]) of the ragged, part-mono, outlier-laden windows of
tests/field_windows.py in turn, each at first, middle and last positions, solved like the main batch.

Spec key "alt": one further batch under the alternative configuration of tests/alt_config.py (a context of its own): the field windows
generated and filled at that configuration, in turn over 32 positions (or spec["alt_sizes"]), reported under "alt32" (row N: also "alt257"
and "alt2049").

Spec keys "const" and "vins": two further resident batches of the windows of tests/const_windows.py (the block-constancy masks the reference
produces; leg and IMU-only windows apart, a batch holds one IMU factor kind), in turn over 32 positions (or spec["const_sizes"] /
spec["vins_sizes"]), the td-estimating window of each set at position 6 where the row runs 23-column rows, reported under "const32" /
"vins32". Spec key "const_alone": the named leg windows each in a batch of their own, under "alone_<name>".

Spec keys "frames" and "vframes": two further resident batches of the windows of tests/frame_windows.py (one window for every frame count
from 2 to 11; leg and IMU-only windows apart), placed by frame_windows.batch_of over 32 positions (or spec["frames_sizes"] /
spec["vframes_sizes"]), reported under "frames32" / "vframes32". Spec key "frames_alone": the named leg windows each in a batch of their
own, under "falone_<name>".

Also importable (no GPU): the window set and its layout, which the test solves with the oracle."""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

ITERS = 4          # fixed trust-region iterations of the main solves (the partial-window tests' count)
FAR_ITERS = 12
FAR = dict(sig_p=1.0, sig_theta=0.4, sig_lambda_rel=0.9, sig_v=1.0, sig_ba=0.3, sig_bg=0.05)   # (tests/_forms_worker.py)
N_SPECIAL_FRAMES = {"partial4": 4, "partial8": 8}


def _filled(cfg, ocfg, L, seed, prior=True, **kw):
    from cerberus_amd import synth
    from oracle import oracle_py as O
    prm = synth.default_params(n_landmarks=L, seed=seed, with_prior=prior)
    for k, v in kw.items():
        setattr(prm, k, v)
    w = synth.make_window(cfg, params=prm)
    O.fill_preint(ocfg, w)
    return w


def _truncate(w, F):
    """First F frames (tests/test_gpu_parity.py: no prior, leg biases constant, landmarks with at least two observations left)."""
    keep = [l for l in range(w.L) if w.lm_start_frame[l] + 2 <= F]
    obs, st, off, sf = [], [], [0], []
    for l in keep:
        o0, o1 = w.lm_obs_offset[l], w.lm_obs_offset[l + 1]
        K = min(o1 - o0, F - w.lm_start_frame[l])
        obs.append(w.obs[o0:o0 + K]); st.append(w.obs_is_stereo[o0:o0 + K]); off.append(off[-1] + K); sf.append(w.lm_start_frame[l])
    w.L, w.n_obs = len(keep), off[-1]
    w.lm_start_frame = np.array(sf, np.int32); w.lm_obs_offset = np.array(off, np.int32)
    w.obs = np.ascontiguousarray(np.concatenate(obs)); w.obs_is_stereo = np.ascontiguousarray(np.concatenate(st))
    w.inv_depth = np.ascontiguousarray(w.inv_depth[keep])
    w.F = F
    w.prior.struct.valid = 0
    w.leg_bias_const = 1
    return w


def _no_landmarks(w):
    w.L, w.n_obs = 0, 0
    w.lm_start_frame = np.zeros(0, np.int32); w.lm_obs_offset = np.zeros(1, np.int32)
    w.obs = np.zeros((0, 11)); w.obs_is_stereo = np.zeros(0, np.uint8); w.inv_depth = np.zeros(0)
    return w


def specials(cfg, ocfg):
    """The windows every row checks, by name (fresh objects: the oracle solves its own copies)."""
    S = {}
    S["bench0"] = _filled(cfg, ocfg, 200, 20260925)
    S["bench1"] = _filled(cfg, ocfg, 200, 20260926)
    S["no_prior"] = _filled(cfg, ocfg, 40, 61, prior=False)
    S["partial4"] = _truncate(_filled(cfg, ocfg, 60, 17), 4)
    S["partial8"] = _truncate(_filled(cfg, ocfg, 60, 17), 8)
    S["skip4"] = _filled(cfg, ocfg, 40, 13)
    S["skip4"].preint[4, 0] = 11.0   # sum_dt of interval (4, 5) > 10 s: no IMU factor there
    S["no_lm"] = _no_landmarks(_filled(cfg, ocfg, 1, 77))
    S["lm7"] = _filled(cfg, ocfg, 7, 2)
    S["lm500"] = _filled(cfg, ocfg, 500, 3)   # more than 64 landmarks per start frame: multi-chunk groups
    return S


def td_window(cfg, ocfg):
    w = _filled(cfg, ocfg, 40, 5)
    w.td_const = 0
    return w


def far_windows(cfg, ocfg):
    return {"far42": _filled(cfg, ocfg, 40, 42, **FAR), "far51": _filled(cfg, ocfg, 40, 51, **FAR)}


def special_positions(W, n):
    """Positions of the n special windows: the first n, n around the middle and the last n (W >= 3 n)."""
    assert W >= 3 * n
    m = W // 2 - n // 2
    return [list(range(n)), list(range(m, m + n)), list(range(W - n, W))]


def layout(S, W, pad_names=("bench0", "bench1"), extra=None):
    """The batch: the specials (dict order) at special_positions, every other position a twin of a pad window in turn; extra: {position:
    window} replaces pads."""
    names = list(S)
    pos = special_positions(W, len(names))
    at = {}
    for block in pos:
        for p, nm in zip(block, names):
            at[p] = nm
    ws, k = [], 0
    for p in range(W):
        if p in at:
            ws.append(S[at[p]] if p == pos[0][names.index(at[p])] else S[at[p]].twin())
        else:
            nm = pad_names[k % len(pad_names)]; k += 1
            ws.append(extra[p] if extra and p in extra else S[nm].twin())
    return ws, pos


def digest(w):
    h = hashlib.sha1()
    for a in w.state_arrays():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _summ(s):
    return {"iterations": s.iterations, "successful": s.num_successful, "termination": s.termination, "final_cost": s.final_cost,
            "cost_trace": list(s.cost_trace[:s.iterations + 1])}


def _solve_resident(ctx, ws, opts, keep, n_solves=3):
    """One batch, n_solves solves with reset in between: the first is plain launches, the later ones replay the captured sequence."""
    from cerberus_amd import api
    init = [w.clone_state() for w in ws]
    b = api.Batch(ctx, ws)
    out = []
    try:
        for i in range(n_solves):
            if i:
                b.reset()
            b.solve(opts)
            summ = b.download()
            r = {"path": b.path(), "digest": [digest(w) for w in ws], "summ": [_summ(s) for s in summ]}
            if i == 0:
                r["state"] = {str(p): [a.tolist() for a in ws[p].state_arrays()] for p in keep}
            out.append(r)
    finally:
        b.close()
    for w, s0 in zip(ws, init):
        w.set_state(s0)
    return out


def field_batch(FS, W, with_td):
    """W field windows in turn (tests/field_windows.batch_of), the td-estimating one at position 6 where the row runs 23-column rows."""
    import field_windows as FW
    return FW.batch_of(FS, W, extra={6: ("f40_td", FS["f40_td"])} if with_td else None)


def field_keep(names):
    """The positions whose states the worker prints: every one of a batch of 32, else each window's first, middle and last position."""
    if len(names) <= 32:
        return list(range(len(names)))
    keep = []
    for nm in dict.fromkeys(names):
        at = [p for p, n in enumerate(names) if n == nm]
        keep += [at[0], at[len(at) // 2], at[-1]]
    return sorted(set(keep))


def _solve_host(ctx, ws, opts):
    init = [w.clone_state() for w in ws]
    summ = ctx.solve_windows(ws, opts)
    r = {"digest": [digest(w) for w in ws], "summ": [_summ(s) for s in summ]}
    for w, s0 in zip(ws, init):
        w.set_state(s0)
    return r


def few(S, W):
    """W windows of a few landmarks: the specials at their positions, every fourth other position a twin of the 7-landmark window and the
    rest twins of the one without landmarks (a window's landmarks take at least one packed wave of their own: so the batch stays at
    most 256 packed waves)."""
    names = list(S)
    pos = special_positions(W, len(names))
    at = {p: nm for block in pos for p, nm in zip(block, names)}
    ws, k = [], 0
    for p in range(W):
        if p in at:
            ws.append(S[at[p]] if p == pos[0][names.index(at[p])] else S[at[p]].twin())
        else:
            ws.append((S["lm7"] if k % 4 == 1 else S["no_lm"]).twin()); k += 1
    return ws, pos


def main():
    from cerberus_amd import api, synth
    from oracle import oracle_py as O
    spec = json.loads(sys.argv[1])
    cfg = synth.default_config()
    ocfg = O.config_from(cfg)
    ctx = api.Context(cfg, 0)
    if "compact" in spec:
        ctx.set_compact_rows(spec["compact"])
    S = specials(cfg, ocfg)
    opts = api.default_solve_opts(True, ITERS)
    res = {}
    for W, is_few in [(W, False) for W in spec.get("sizes", [32])] + [(W, True) for W in spec.get("few_sizes", [])]:
        extra = None
        if spec.get("td"):
            extra = {len(S): td_window(cfg, ocfg)}   # the first pad position
        if is_few:
            ws, pos = few(S, W)
        else:
            ws, pos = layout(S, W, extra=extra)
        keep = sorted({p for block in pos for p in block} | set(extra or {}))
        r = {"W": W, "positions": pos}
        if spec.get("host_only"):
            r["host"] = _solve_host(ctx, ws, opts)
        else:
            r["solves"] = _solve_resident(ctx, ws, opts, keep)
            if spec.get("host"):
                r["host"] = _solve_host(ctx, ws, opts)
        res[("few%d" if is_few else "%d") % W] = r
    if spec.get("far"):
        o = api.default_solve_opts(True, FAR_ITERS)
        o.initial_trust_region_radius = 1e8
        fw = list(far_windows(cfg, ocfg).values())
        res["far"] = {"solves": _solve_resident(ctx, fw, o, [0, 1])}
    if spec.get("field"):
        import field_windows as FW
        FS = FW.field_set(cfg, ocfg)
        for W in spec.get("field_sizes", [32]):
            ws, names = field_batch(FS, W, bool(spec.get("td")) or spec.get("compact") == 0)
            res["field%d" % W] = {"W": W, "names": names, "solves": _solve_resident(ctx, ws, opts, field_keep(names))}
    if spec.get("const") or spec.get("vins") or spec.get("const_alone"):
        import time
        import const_windows as CW
        with_td = bool(spec.get("td")) or spec.get("compact") == 0
        for key, make in (("const", CW.const_set), ("vins", CW.vins_set)):
            if not spec.get(key):
                continue
            t0 = time.perf_counter()
            CS = make(cfg, ocfg)
            for W in spec.get(key + "_sizes", [32]):
                ws, names = CW.batch_of(CS, W, with_td)
                res["%s%d" % (key, W)] = {"W": W, "names": names, "solves": _solve_resident(ctx, ws, opts, field_keep(names))}
                res["%s%d" % (key, W)]["seconds"] = time.perf_counter() - t0   # (what this batch adds to the row, window generation included)
                t0 = time.perf_counter()
        for nm in spec.get("const_alone", []):
            res["alone_" + nm] = {"W": 1, "names": [nm], "solves": _solve_resident(ctx, [CW.leg_window(cfg, ocfg, nm)], opts, [0])}
    if spec.get("frames") or spec.get("vframes") or spec.get("frames_alone"):
        import time
        import frame_windows as FR
        for key, make in (("frames", FR.leg_set), ("vframes", FR.vins_set)):
            if not spec.get(key):
                continue
            t0 = time.perf_counter()
            GS = make(cfg, ocfg)
            for W in spec.get(key + "_sizes", [32]):
                ws, names = FR.batch_of(GS, W)
                res["%s%d" % (key, W)] = {"W": W, "names": names, "solves": _solve_resident(ctx, ws, opts, field_keep(names))}
                res["%s%d" % (key, W)]["seconds"] = time.perf_counter() - t0   # (what this batch adds to the row, window generation included)
                t0 = time.perf_counter()
        for nm in spec.get("frames_alone", []):
            res["falone_" + nm] = {"W": 1, "names": [nm], "solves": _solve_resident(ctx, [FR.leg_window(cfg, ocfg, nm)], opts, [0])}
    ctx.close()
    if spec.get("alt"):
        import alt_config
        import field_windows as FW
        acfg = alt_config.alt_config(cfg)
        oacfg = O.config_from(acfg)
        actx = api.Context(acfg, 0)
        if "compact" in spec:
            actx.set_compact_rows(spec["compact"])
        import time
        t0 = time.perf_counter()
        AS = FW.field_set(acfg, oacfg)
        for W in spec.get("alt_sizes", [32]):
            ws, names = field_batch(AS, W, bool(spec.get("td")) or spec.get("compact") == 0)
            res["alt%d" % W] = {"W": W, "names": names, "solves": _solve_resident(actx, ws, opts, field_keep(names), n_solves=2)}
            res["alt%d" % W]["seconds"] = time.perf_counter() - t0   # (what this batch adds to the row, window generation included)
            t0 = time.perf_counter()
        actx.close()
    print("PATHS_JSON " + json.dumps(res))


if __name__ == "__main__":
    main()
