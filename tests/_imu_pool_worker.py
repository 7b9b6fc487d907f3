"""Worker of test_imu_pool_form.py: solves one small batch through a resident batch under the tuning switches the environment pins (the
library reads them once per process) and prints, as JSON, the descriptor of the solve (vilo_debug_batch_path), every window's final
state, digest and summary, and on request the priors of vilo_batch_marginalize (mode 0 of k_imu_linearize: the whitened block).

Also importable (no GPU): the window set of a case, which the test solves with the oracle."""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

ITERS = 4   # fixed trust-region iterations (tests/_paths_worker.py)
L = 12      # landmarks per window: the IMU kernels are what the cases are about

# case: W windows of seeds 500 + i; use_leg of all of them (a batch holds one IMU factor kind: vilo_batch_create refuses a mix);
# skip: {window: interval without a factor}. W * 5 pairs: 5 (the permutation's ragged identity branch), 35 (one permuted group of 32
# plus a tail), 65 (two groups plus a tail).
CASES = {
    "w1": dict(W=1, use_leg=1, skip={}),
    "w7": dict(W=7, use_leg=1, skip={}),
    "w13": dict(W=13, use_leg=1, skip={}),
    "w7_imu": dict(W=7, use_leg=0, skip={}),
    # interval 4 is the first factor of pair (4, 5), interval 7 the second of pair (6, 7); window 6: both factors of pair (2, 3)
    "w7_skip": dict(W=7, use_leg=1, skip={1: [4], 3: [7], 6: [2, 3]}),
    "w7_imu_skip": dict(W=7, use_leg=0, skip={0: [0], 2: [9], 5: [5]}),
}


def windows(cfg, ocfg, case):
    from cerberus_amd import synth
    from oracle import oracle_py as O
    c = CASES[case]
    ws = []
    for i in range(c["W"]):
        w = synth.make_window(cfg, params=synth.default_params(n_landmarks=L, seed=500 + i, with_prior=True))
        O.fill_preint(ocfg, w)
        if not c["use_leg"]:
            w.use_leg, w.leg_bias_const = 0, 1
        for k in c["skip"].get(i, []):   # sum_dt > 10 s: no IMU factor on the interval
            w.preint[k, 0] = 11.0
            w.preint_imu[k, 0] = 11.0
        ws.append(w)
    return ws


def digest(w):
    import hashlib
    h = hashlib.sha1()
    for a in w.state_arrays():
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def _summ(s):
    return {"iterations": s.iterations, "successful": s.num_successful, "termination": s.termination, "final_cost": s.final_cost,
            "cost_trace": list(s.cost_trace[:s.iterations + 1])}


def main():
    from cerberus_amd import api, synth
    from cerberus_amd.synth import PriorData
    from oracle import oracle_py as O
    spec = json.loads(sys.argv[1])
    cfg = synth.default_config()
    ocfg = O.config_from(cfg)
    ctx = api.Context(cfg, 0)
    ws = windows(cfg, ocfg, spec["case"])
    res = {}
    b = api.Batch(ctx, ws)
    try:
        b.solve(api.default_solve_opts(True, ITERS))
        summ = b.download()
        res["path"] = b.path()
        res["digest"] = [digest(w) for w in ws]
        res["summ"] = [_summ(s) for s in summ]
        res["state"] = [[a.tolist() for a in w.state_arrays()] for w in ws]
        if spec.get("marg"):
            # at the solved states (the windows' arrays are the host copy of the device state after download()): the test hands the
            # oracle the same states
            pri = [PriorData() for _ in ws]
            b.marginalize([0] * len(ws), pri)
            res["prior"] = [{"n": p.n, "valid": int(p.struct.valid), "blocks": [list(x) for x in p.blocks()],
                             "J0": p.J0[:p.n * p.n].tolist(), "r0": p.r0[:p.n].tolist()} for p in pri]
    finally:
        b.close()
    ctx.close()
    print("IMU_POOL_JSON " + json.dumps(res))


if __name__ == "__main__":
    main()
