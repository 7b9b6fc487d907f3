"""Test helper: the cost gradient and Gauss-Newton diagonal of a window (include/vilo_gpu.h, "cost gradient") in the arrays
vilo_batch_gradient returns, from ref_gradient.cost_and_gradient — the factor classes' own Evaluate(), the oracle's or inside
`with ref_py.as_oracle():` the compiled reference's; nothing of the kernels under test — and the window record recomputed in numpy.
Layout of the 222 state entries: pose 11 x 6, speed-bias 11 x 9, leg bias 11 x 4, extrinsics 2 x 6, td."""
import numpy as np

import ref_gradient as RG

NS = 222
# (kind, first entry, local size, blocks): VILO_BLK_* 0 pose, 1 speed-bias, 2 leg bias, 3 extrinsic, 4 td
BLOCKS = ((0, 0, 6, 11), (1, 66, 9, 11), (2, 165, 4, 11), (3, 209, 6, 2), (4, 221, 1, 1))

# FP64 floor of the definition in the metric below, as tests/test_gradient.py::test_fp64_floor_measured prints it (the larger of the
# one-ulp and the oracle-against-reference figure over its windows, rounded up), and the GPU tolerances: ten times the floor
FLOOR_G, FLOOR_H = 5e-9, 6e-13
TOL_G, TOL_H = 10 * FLOOR_G, 10 * FLOOR_H


def position(kind, index, comp=0):
    for k, first, size, _ in BLOCKS:
        if k == kind:
            return first + size * index + comp
    raise KeyError(kind)


def free_mask(w):
    """which of the 222 entries are free local coordinates: frames below n_frames; not ex_const / td_const / leg_bias_const; no leg bias
    when use_leg == 0"""
    m = np.zeros(NS, bool)
    for kind, first, size, n in BLOCKS:
        for i in range(n):
            on = i < w.F if kind in (0, 1, 2) else True
            if kind == 2 and (w.leg_bias_const or not w.use_leg):
                on = False
            if kind == 3 and w.ex_const:
                on = False
            if kind == 4 and w.td_const:
                on = False
            m[first + size * i:first + size * (i + 1)] = on
    return m


def flatten(w, g, h):
    """ref_gradient's dictionaries -> (state_grad [222], state_diag [222], lm_grad [L], lm_diag [L]); constant and absent blocks zero"""
    free = free_mask(w)
    out = []
    for d in (g, h):
        s, lm = np.zeros(NS), np.zeros(w.L)
        for key, v in d.items():
            if key[0] == "lam":
                lm[key[1]] = np.atleast_1d(v)[0]
            else:
                p = position(key[0], key[1])
                v = np.atleast_1d(v).ravel()
                s[p:p + v.size] = v
        s[~free] = 0.0
        out.append((s, lm))
    return out[0][0], out[1][0], out[0][1], out[1][1]


def record(free, sg, sd, lg, ld):
    """the window record from the arrays: norms over the free entries, the arg-max as the first entry of the largest |g| in the order
    state entries, then landmarks"""
    gv = np.concatenate([sg[free], lg])
    hv = np.concatenate([sd[free], ld])
    pos = np.concatenate([np.flatnonzero(free), NS + np.arange(lg.size)])
    r = dict(n_free=int(gv.size), max_norm=0.0, norm=0.0, scaled_max=0.0, argmax_kind=-1, argmax_index=-1, argmax_component=-1)
    if gv.size == 0:
        return r
    a = np.abs(gv)
    p = int(pos[int(np.argmax(a))])   # (argmax: the first of equal maxima)
    r["max_norm"], r["norm"] = float(a.max()), float(np.sqrt((gv * gv).sum()))
    ok = hv > 0
    r["scaled_max"] = float((a[ok] / np.sqrt(hv[ok])).max()) if ok.any() else 0.0
    if p >= NS:
        r["argmax_kind"], r["argmax_index"], r["argmax_component"] = 5, p - NS, 0
    else:
        for kind, first, size, n in BLOCKS:
            if first <= p < first + size * n:
                r["argmax_kind"], r["argmax_index"], r["argmax_component"] = kind, (p - first) // size, (p - first) % size
    return r


def window_gradient(cfg, w, huber_delta=None):
    """(cost, state_grad, state_diag, lm_grad, lm_diag, record) of window w at its state arrays"""
    cost, g, h = RG.cost_and_gradient(cfg, w, huber_delta)
    sg, sd, lg, ld = flatten(w, g, h)
    return cost, sg, sd, lg, ld, record(free_mask(w), sg, sd, lg, ld)


def errors(w, got, ref):
    """got, ref: (state_grad, state_diag, lm_grad, lm_diag). Returns (err_g, err_h): max |dg_i| / max(sqrt(h_i), |g_i|) and max |dh_i| / h_i
    over the free entries and the landmarks (h of the reference)."""
    free = free_mask(w)
    dg = np.concatenate([(got[0] - ref[0])[free], got[2] - ref[2]])
    dh = np.concatenate([(got[1] - ref[1])[free], got[3] - ref[3]])
    g = np.concatenate([ref[0][free], ref[2]])
    h = np.concatenate([ref[1][free], ref[3]])
    if g.size == 0:
        return 0.0, 0.0
    return float((np.abs(dg) / np.maximum(np.sqrt(h), np.abs(g))).max()), float((np.abs(dh) / h).max())
