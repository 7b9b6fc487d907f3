"""Worker of tests/test_batch_sequences_gpu.py::test_row_G_environment: every fixed sequence on the leg batch under the tuning switches the
environment pins (the library reads them once per process); prints, as JSON, "ok" or the failed assertion per sequence and the descriptor
of the last solve."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    import batch_model as M
    import test_batch_sequences_gpu as G
    from cerberus_amd import api, synth
    from oracle import oracle_py as O
    cfg = synth.default_config()
    ocfg = O.config_from(cfg)
    ctx = api.Context(cfg, 0)
    distinct = list(M.leg_windows(cfg, ocfg).values())
    res, path = {}, None
    for name in M.SEQUENCES:
        try:
            r = G.Runner(ctx, cfg, ocfg, distinct, G.SIZES["leg"], name)
            try:
                while not r.done():
                    r.step()
                path = r.dev.b.path()
            finally:
                r.close()
            res[name] = "ok"
        except (AssertionError, api.ViloError) as e:
            res[name] = repr(e)[:600]
    ctx.close()
    print("SEQUENCES_JSON " + json.dumps({"results": res, "path": path}))


if __name__ == "__main__":
    main()
