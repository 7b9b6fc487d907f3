"""Helper and worker of test_chain_fact.py: the batches that test solves, and one function that solves them with a given solver form and
returns everything compared — states, summaries, retries and the chain's hand-over buffers M_k / T_A(k) / T(k) through vilo_debug_fetch.
As a program it solves them with the three-stage form under whatever the environment pins (VILO_CHAIN_SINGLE is read once per process)
and writes the results to the .npz named on its command line."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

from cerberus_amd import api, synth  # noqa: E402

ITERS = 4
MIXED_W = (1, 3, 4, 5, 9)
# the mixed batch by position: in the first wave the four 16-lane groups see (11 frames, prior, default mask), (11, prior, ragged field
# window), (8 frames, no prior), (11 frames, no prior, kb < 0); the second wave starts with a constant-leg-bias mask
MIXED = ("g40", "f40", "f60_partial8", "f130_noprior", "c40_lb", "c40_ex_lb", "f60_partial8", "g40b", "f40")


def _gen(cfg, seed, L=40, prior=True, **kw):
    prm = synth.default_params(n_landmarks=L, seed=seed, with_prior=prior)
    for k, v in kw.items():
        setattr(prm, k, v)
    return synth.make_window(cfg, params=prm)


def mixed_windows(cfg, W):
    import const_windows as CW
    import field_windows as FW
    from oracle import oracle_py as O
    ocfg = O.config_from(cfg)
    out = []
    for name in MIXED[:W]:
        if name == "g40":
            out.append(FW._filled(cfg, ocfg, 40, 42))
        elif name == "g40b":
            out.append(FW._filled(cfg, ocfg, 40, 48))
        elif name.startswith("c"):
            out.append(CW.leg_window(cfg, ocfg, name))
        else:
            out.append(FW.field_window(cfg, ocfg, name))
    return out


FRAMES_W = 2049   # the frames batch of tests/frame_windows.py at the size whose plan names the three-stage form by itself
KEEP = {}         # {case: positions whose results are kept}; a case that is not here keeps every window


def frames_windows(cfg, W):
    """frame_windows.batch_of's leg batch: every frame count from 2 to 11, four different ones in every wave of k_chain_fact, (2, 11, 3, 10)
    in the first. Kept: the first 32 positions (one turn of the placement), the last 33 (the last wave holds one window) and each window's
    first, middle and last position."""
    import _paths_worker as P
    import frame_windows as FR
    from oracle import oracle_py as O
    ws, names = FR.batch_of(FR.leg_set(cfg, O.config_from(cfg)), W)
    return ws, sorted(set(range(32)) | set(range(W - 33, W)) | set(P.field_keep(names))), names


FAR = dict(sig_p=1.0, sig_theta=0.4, sig_lambda_rel=0.9, sig_v=1.0, sig_ba=0.3, sig_bg=0.05)


def cases(cfg, ctx):
    """{case: (windows, opts)}; generator windows are preintegrated by ctx, the field windows come filled by the oracle."""
    out = {}
    for W in MIXED_W:
        out["mixed%d" % W] = (mixed_windows(cfg, W), api.default_solve_opts(True, ITERS))
    ws, KEEP["frames%d" % FRAMES_W], _ = frames_windows(cfg, FRAMES_W)
    out["frames%d" % FRAMES_W] = (ws, api.default_solve_opts(True, ITERS))
    ws = [_gen(cfg, 42) for _ in range(8)]
    ctx.preintegrate_windows(ws)
    out["equal8"] = (ws, api.default_solve_opts(True, ITERS))
    # tests/_forms_worker.py's escalation: the window without a prior fails its factorisation at the initial mu under these options
    o = api.default_solve_opts(True, ITERS)
    o.min_lm_diagonal = o.max_lm_diagonal = 1e-12
    healthy = [(42, 40), (48, 90), (51, 12)]
    ws = [_gen(cfg, s, L) for s, L in healthy]
    ctx.preintegrate_windows(ws)
    out["healthy3"] = (ws, o)
    for pos in range(4):
        ws = [_gen(cfg, s, L) for s, L in healthy]
        ws.insert(pos, _gen(cfg, 60, prior=False))
        ctx.preintegrate_windows(ws)
        out["fail_at%d" % pos] = (ws, o)
    # far-off starts with a huge radius (runs of rejected steps, each keeping its linearisation) between plain windows, in one wave
    o = api.default_solve_opts(True, 12)
    o.initial_trust_region_radius = 1e8
    ws = [_gen(cfg, 42), _gen(cfg, 42, **FAR), _gen(cfg, 48, L=90), _gen(cfg, 51, **FAR)]
    ctx.preintegrate_windows(ws)
    out["rejected"] = (ws, o)
    return out


def tk_written(F):
    """Mask over a window's [TK_N] hand-over buffer of the entries every form writes: frames below F, tiles from chain_x_lo of a frame
    above the prior's (the prior's frame is 0 or none in these windows, where chain_x_lo is the same expression), rows 0 .. 12, and the
    80 entries of the reduced right-hand side."""
    m = np.zeros(14208, bool)
    lk = np.arange(64) >> 4
    for k in range(F):
        x_lo = max(0, (6 * (k - 1)) >> 4)
        for X in range(x_lo, 5):
            for kk in range(4):
                m[1280 * k + (X * 4 + kk) * 64 + np.arange(64)] = (kk < 3) | (lk == 0)
    m[14080:14160] = True
    return m


def solve_case(ctx, ws, opts, keep=None):
    """[result of window i for i in keep (None: every window)], the batch's descriptor."""
    b = api.Batch(ctx, ws)
    try:
        b.solve(opts)
        summ = b.download()
        path = b.path()
        res = []
        for i, (w, s) in enumerate(zip(ws, summ)):
            if keep is not None and i not in keep:
                continue
            F = int(w.F)
            r = {"state": np.concatenate([np.asarray(a, np.float64).ravel() for a in w.state_arrays()]),
                 "cost": np.array(s.cost_trace[:s.iterations + 1]), "radius": np.array(s.radius_trace[:s.iterations + 1]),
                 "summary": np.array([s.iterations, s.num_successful, s.termination], np.int64),
                 "retries": np.array([int(b.fetch(10, i)[18:24].view(np.int32)[10])], np.int64),
                 "M": b.fetch(18, i, 1859)[:169 * F], "TA": b.fetch(19, i, 1859)[:169 * F], "T": b.fetch(20, i, 14208)[tk_written(F)]}
            res.append(r)
    finally:
        b.close()
    return res, path


def solve_all(form):
    """{case/window index/field: array} of every case with solver form `form` (a fresh context)."""
    cfg = synth.default_config()
    ctx = api.Context(cfg, 0)
    ctx.set_solver_form(form)
    flat = {}
    all_cases = cases(cfg, ctx)
    for name, (ws, opts) in all_cases.items():
        keep = KEEP.get(name)
        res, path = solve_case(ctx, ws, opts, None if keep is None else set(keep))
        assert path["solver"] == form, path
        for i, r in zip(keep if keep is not None else range(len(res)), res):
            for k, v in r.items():
                flat["%s/%d/%s" % (name, i, k)] = v
    # which chain kernels this process launches: one more solve of a case with the per-kernel timing on (its launch counts)
    import ctypes as C
    L = api.lib()
    L.vilo_set_profiling(ctx.h, 1)
    ws, opts = all_cases["equal8"]
    b = api.Batch(ctx, ws)
    try:
        b.solve(opts)
        b.download()
    finally:
        b.close()
    ms = (C.c_double * 32)()
    launches = (C.c_longlong * 32)()
    nk = L.vilo_get_kernel_times(ctx.h, ms, launches, 32)
    L.vilo_kernel_name.restype = C.c_char_p
    count = {L.vilo_kernel_name(i).decode(): int(launches[i]) for i in range(nk)}
    L.vilo_set_profiling(ctx.h, 0)
    flat["launches/k_chain_fact"] = np.array([count["k_chain_fact"]], np.int64)
    flat["launches/k_chain"] = np.array([count["k_chain"]], np.int64)
    ctx.close()
    return flat


if __name__ == "__main__":
    np.savez(sys.argv[1], **solve_all("split"))
    print("CHAIN_FACT_WORKER_DONE")
