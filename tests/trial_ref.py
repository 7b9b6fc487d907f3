"""Test helper (no test in it): the definition of vilo_batch_trial_cost (include/vilo_gpu.h, "the cost at up to 16 trial steps") in numpy
and the oracle, one window at a time: retract_ref.retract to each trial state, then the oracle's cost there as
tests/test_retract.py::cost_after evaluates it (a twin at that state, O.window_cost), the status rules and `best`. With parts=True the
record's parts come from resid_ref.window_residuals at the same state (per-factor oracle evaluations, summed in numpy's order)."""
import numpy as np

import retract_ref as RR

OK, NUMERIC, INVALID, NOT_FINITE = 0, 1, 2, 3   # vilo_trial_record.status
FIELDS = ("cost", "visual_cost", "imu_cost", "prior_cost", "cost_change", "n_negative_depth", "status")

# The oracle's cost of one state in two orders of summation: O.window_cost (Ceres' order over the residual blocks) against
# resid_ref.window_residuals (prior + intervals + landmarks, numpy's sums), |a - b| / a at the trial states tests/test_trial_cost_gpu.py
# uses (steps of 1e-2, alpha in [0.5, 1.5)), the largest over retract_ref's six kinds and three steps each, as
# tests/test_trial_cost.py::test_floor_of_the_oracle_cost_in_two_orders measures it. The GPU test holds ten times the figure.
TRIAL_MEASURED = 2.9e-15   # (the 130-landmark IMU-only window; 4.4e-16 .. 1.6e-15 on the leg kinds)
TRIAL_TOL = 10.0 * TRIAL_MEASURED


def _at(w, arrays, lm_mask):
    t = w.twin()
    t.set_state(arrays)
    if lm_mask is not None and np.asarray(lm_mask).any():
        import mask_ref
        t = mask_ref.delete_landmarks(t, np.asarray(lm_mask))
    return t


def cost_at(ocfg, w, arrays, lm_mask=None, parts=False):
    """dict(cost, and with parts visual_cost, imu_cost, prior_cost) of window w at the given state arrays"""
    from oracle import oracle_py as O
    t = _at(w, arrays, lm_mask)
    out = dict(cost=float(O.window_cost(ocfg, t)))
    if parts:
        import resid_ref
        r = resid_ref.window_residuals(ocfg, t)
        out.update(visual_cost=r["visual_cost"], imu_cost=float(r["imu_cost"].sum()), prior_cost=r["prior_cost"], cost_parts=r["cost"])
    return out


def best_of(status, cost, cost_change):
    """the smallest k of status OK with the lowest cost among those with cost_change > 0, or -1"""
    bk = -1
    for k in range(len(status)):
        if status[k] == OK and cost_change[k] > 0 and (bk < 0 or cost[k] < cost[bk]):
            bk = k
    return bk


def trial_cost(ocfg, w, state_steps, lm_steps, alphas, pose_plus=RR.pose_plus_np, lm_mask=None, parts=False):
    """(records, base, best, states) of one window: records a dict of [K] arrays over FIELDS (+ the parts' sum "cost_parts" with parts),
    base the same dict of scalars at the window's own state (cost_change 0), states the K trial states' arrays (None where NUMERIC).
    state_steps [K, 222], lm_steps [K, L], alphas [K]."""
    K = len(alphas)
    base = cost_at(ocfg, w, w.state_arrays(), lm_mask, parts)
    free_lm = RR.applied(w, lm_mask)[1]
    base.update(cost_change=0.0, n_negative_depth=int((w.inv_depth[free_lm] < 0).sum()),
                status=OK if np.isfinite(base["cost"]) else NOT_FINITE)
    names = [f for f in FIELDS if parts or f in ("cost", "cost_change", "n_negative_depth", "status")] + (["cost_parts"] if parts else [])
    rec = {f: np.full(K, np.nan) if f not in ("n_negative_depth", "status") else np.zeros(K, np.int32) for f in names}
    states = []
    for k in range(K):
        arrays, r = RR.retract(w, state_steps[k], lm_steps[k], alphas[k], pose_plus, lm_mask=lm_mask)
        if r["status"] != RR.OK:
            rec["status"][k] = NUMERIC
            states.append(None)
            continue
        states.append(arrays)
        c = cost_at(ocfg, w, arrays, lm_mask, parts)
        for f, v in c.items():
            rec[f][k] = v
        rec["cost_change"][k] = base["cost"] - c["cost"]
        rec["n_negative_depth"][k] = int((arrays[5][free_lm] < 0).sum())
        rec["status"][k] = OK if np.isfinite(c["cost"]) else NOT_FINITE
    return rec, base, best_of(rec["status"], rec["cost"], rec["cost_change"]), states


# ---- the steps the trial-cost tests share ----
def steps(ws, K, seed, masks=None):
    """(state_step [W, K, 222], lm_step [K sum L] in the call's layout, alpha [W, K], per-window [K, L] landmark steps): RR.random_step at
    scale 1e-2 with NaN wherever the call must not read, alpha in [0.5, 1.5)"""
    rng = np.random.default_rng(seed)
    ss, blocks = np.zeros((len(ws), K, RR.NS)), []
    for i, w in enumerate(ws):
        ls = np.zeros((K, w.L))
        for k in range(K):
            ss[i, k], ls[k] = RR.random_step(w, rng, lm_mask=None if masks is None else masks[i])
        blocks.append(ls)
    return ss, np.concatenate([b.ravel() for b in blocks]), 0.5 + rng.random((len(ws), K)), blocks
