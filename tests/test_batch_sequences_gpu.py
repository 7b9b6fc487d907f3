"""GPU (-m gpu): sequences of state-changing calls on one resident batch, held against tests/batch_model.py after every call.

Each fixed sequence of batch_model.SEQUENCES runs on a batch of 32 (the eight leg windows of batch_model.leg_windows, each at four
positions) and on a batch of 8 (the four IMU-only windows, twice), every solve ITERS fixed iterations, under Context.set_solver_form auto,
wave and split, and once in a child process under row G's environment of tests/test_kernel_paths.py (tests/_sequences_worker.py).

After every call every component of the batch is read back (Device.observe):
  the current state and the summaries with download; the uploaded copy with reset + download; the snapshot, where the model says there is
  one, with restore_state + download; then set_state of every window puts the current state back, and a last download holds that it did;
  the records with fetch(13) (fetch(16) for IMU-only records) and fetch(15); the mask as the mask_out of an OR round of an all-zero mask.
(The uploaded copy is not read through save_state: that would overwrite the one snapshot slot, which is itself under test.)
A component the model says the call leaves alone must be bytewise what it was; a component it changes must equal the model's, bit for bit
where the model says so, else within the bound the call's own GPU test uses (Outcome.approx names the file). The positions of one window
must agree bytewise in every component. device_bytes()[1] may grow only at a batch's first call of a kind.

At the end of a sequence a fresh batch is created from the downloaded state, the fetched records and the mask; both are solved: the
used batch's solve is a replay where it has solved before, the fresh batch's is plain launches, and states and summaries must be bitwise
equal; the used batch's result is held against the oracle's solve of the model's final windows like every other solve (1e-8).

Measured on an MI355X: the whole file 93 s (242 cases, the child under row G's switches 16 s)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import batch_model as M

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = ["auto", "wave", "split"]
SIZES = {"leg": 32, "imu": 8}
UNSUPPORTED = "vilo error -5"


@pytest.fixture(scope="module")
def ctx(cfg):
    from cerberus_amd import api
    c = api.Context(cfg, 0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def sets(cfg, ocfg):
    return {"leg": list(M.leg_windows(cfg, ocfg).values()), "imu": list(M.imu_windows(cfg, ocfg).values())}


class Device:
    """A resident batch of W positions over the distinct windows, and the calls of a sequence on it."""

    def __init__(self, ctx, distinct, W, pos=None):
        from cerberus_amd import api
        self.ctx, self.distinct = ctx, distinct
        self.pos = M.positions(len(distinct), W) if pos is None else pos
        self.ws = [distinct[d].twin() for d in self.pos]
        self.off = np.concatenate([[0], np.cumsum([w.L for w in self.ws])]).astype(np.int64)
        self.b = api.Batch(ctx, self.ws)
        self.opts = api.default_solve_opts(True, M.ITERS)
        self.holders = [w.twin() for w in self.ws]
        self.solves = 0
        self.leg = bool(distinct[0].use_leg)
        self.samples_on, self.mask_now, self.priors_held = False, None, 0   # (the runner keeps the first two current)

    def close(self):
        self.b.close()

    def _trims(self):
        return [M.trim(w, w.state_arrays()) for w in self.ws]

    def observe(self, snapshot):
        """{component: one value per position}"""
        b = self.b
        summ = b.download()
        out = {"state": self._trims(), "summaries": [bytes(s) for s in summ]}
        b.reset(); b.download()
        out["uploaded"] = self._trims()
        if snapshot:
            b.restore_state(); b.download()
            out["snapshot"] = self._trims()
        else:
            out["snapshot"] = [None] * len(self.ws)
        for h, s in zip(self.holders, out["state"]):
            for k, (dst, src) in enumerate(zip(h.state_arrays(), s)):
                if k < 3:
                    dst[:h.F] = src
                else:
                    dst[...] = src
        b.set_state(list(range(len(self.ws))), self.holders)
        b.download()
        assert [M.state_bytes(s) for s in self._trims()] == [M.state_bytes(s) for s in out["state"]], "the observation did not put the state back"
        recs = []
        for p, w in enumerate(self.ws):
            raw = b.fetch(13 if self.leg else 16, p).reshape(10, -1)[:w.F - 1]
            recs.append((raw, b.fetch(15, p).reshape(10, -1)[:w.F - 1].tobytes()))   # (the entries of absent intervals: as they lie)
        out["records"] = recs
        m, _ = b.mask_landmarks(mask=np.zeros(int(self.off[-1]), np.uint8), combine="or")
        out["mask"] = [m[self.off[p]:self.off[p + 1]].copy() for p in range(len(self.ws))]
        return out

    def _hold_priors(self, outs):
        """vilo_batch_marginalize's priors against vilo_marginalize on the downloaded windows (the state the last observation left in the
        windows' arrays by the download before the call, the records fetched now, the model's mask, which the observed runs hold
        equal to the device's) with the masked landmarks removed, as tests/test_mask_gpu.py::test_marginalize_a_masked_batch
        holds a masked batch against the rebuilt one: same blocks, H and b per block pair within 2e-5 of the blocks' diagonals
        (MARGIN_OLD), and bit for bit where that test's reason for it holds. With samples in force the batch integrates its records again first, which the host-window call does
        not: left out there."""
        from cerberus_amd.synth import PriorData
        from marg_exact import block_table, scaled_errors
        import mask_ref
        if self.samples_on:
            return
        n = 0
        for p, w in enumerate(self.ws):
            if w.F != 11:
                continue
            t = w.twin()
            raw = self.b.fetch(13 if self.leg else 16, p).reshape(10, -1)[:w.F - 1]
            if w.use_leg:
                t.preint = w.preint.copy(); t.preint[:w.F - 1] = raw
            else:
                t.preint_imu = w.preint_imu.copy(); t.preint_imu[:w.F - 1] = raw
            m = self.mask_now[p]
            rw = mask_ref.delete_landmarks(t, m) if m.any() else t
            ref = PriorData()
            self.ctx.marginalize(rw, 0, ref)
            pg = outs[p]
            assert pg.struct.valid == ref.struct.valid == 1 and pg.blocks() == ref.blocks(), ("marginalize", p)
            k = ref.n
            Jr = ref.J0_matrix()
            eh, eb, _, _ = scaled_errors(pg, Jr.T @ Jr, Jr.T @ ref.r0[:k], block_table(ref))
            assert max(eh, eb) < 2e-5, ("marginalize", p, eh, eb)
            # Bit for bit where that test's reason holds: deleting landmarks keeps the others' order inside their start-frame chunk while
            # every start frame has one chunk (64 lanes). f70_chunks has 70 landmarks on one start frame: a mask moves landmarks from the
            # second chunk into the first, the sums take another order (measured 3e-14 .. 6e-13 of the blocks' diagonals), and the
            # tolerance above is what holds it.
            if not m.any() or np.bincount(w.lm_start_frame, minlength=11).max() <= 64:
                assert pg.J0_matrix().tobytes() == Jr.tobytes() and pg.r0[:k].tobytes() == ref.r0[:k].tobytes(), ("marginalize", p, "not bit for bit", eh, eb)
            n += 1
        self.priors_held += n

    def per_position(self, values):
        return [values[d] for d in self.pos]

    def run(self, op, inputs):
        """-> (refused, extra keyword arguments for the model's method)"""
        from cerberus_amd import api
        from cerberus_amd.synth import PriorData
        kind, kw = op
        b, extra = self.b, {}
        try:
            if kind == "solve":
                b.solve(self.opts)
                self.solves += 1
            elif kind == "reset":
                b.reset()
            elif kind == "set_samples_on":
                b.set_samples(True)
            elif kind == "set_samples_off":
                b.set_samples(False)
            elif kind == "repropagate":
                r = b.repropagate(point="state", select="all", write=True)
                for p, w in enumerate(self.ws):
                    assert (r.status[p, :w.F - 1] == 0).all(), (p, r.status[p])
            elif kind == "mask":
                want = np.concatenate(self.per_position(inputs["masks"])) if self.off[-1] else np.zeros(0, np.uint8)
                m, _ = b.mask_landmarks(mask=want)
                assert m.tobytes() == want.tobytes()
            elif kind == "mask_or":
                flags = b.residuals().lm_flags
                m, _ = b.mask_landmarks("outlier_flags", combine="or")
                sel = [((flags[self.off[p]:self.off[p + 1]] & 3) != 0).astype(np.uint8) for p in range(len(self.ws))]
                first = {d: sel[p] for p, d in reversed(list(enumerate(self.pos)))}
                assert all(sel[p].tobytes() == first[d].tobytes() for p, d in enumerate(self.pos)), "the selection depends on the position"
                extra["selection"] = [first[d] for d in range(len(self.distinct))]
            elif kind == "clear_mask":
                b.clear_mask()
            elif kind in ("retract", "retract_uploaded"):
                st = self.per_position(inputs["steps"])
                r = b.retract(np.array([s for s, _, _ in st]), np.concatenate([l for _, l, _ in st]), np.array([a for _, _, a in st]),
                              base="uploaded" if kind == "retract_uploaded" else "current")
                assert (r.status == 0).all()
            elif kind == "set_state":
                ids = [p for p, d in enumerate(self.pos) if d in inputs["ids"]]
                b.set_state(ids, [inputs["states"][self.pos[p]] for p in ids])
            elif kind == "save_state":
                b.save_state()
            elif kind == "restore_state":
                b.restore_state()
            elif kind == "gauge_fix":
                assert (b.gauge_fix().status == 0).all()
            elif kind == "triangulate":
                b.triangulate(select="all", write=True, shift=True)
            elif kind == "frame_pose_pnp":
                b.frame_pose_pnp(write=True, step_tolerance=M.pnp_ref.PARITY_STEP_TOLERANCE)
            elif kind == "gyro_bias_align":
                assert (b.gyro_bias_align("record", write=True).status == 0).all()
            elif kind == "dead_reckon":
                sm = self.per_position(inputs["samples"])
                r = b.dead_reckon(np.concatenate(sm), np.concatenate([[0], np.cumsum([len(s) for s in sm])]).astype(np.int32), from_frame=0, write=True)
                assert (r.status == 0).all()
            elif kind == "marginalize":
                outs = [PriorData() for _ in self.ws]
                b.download()   # (the host copy of the device state the call takes; reads only)
                b.marginalize([0 if w.F == 11 else -1 for w in self.ws], outs)
                self._hold_priors(outs)
            elif kind == "residuals":
                b.residuals()
            elif kind == "gradient":
                b.gradient()
            else:
                raise KeyError(kind)
        except api.ViloError as e:
            assert UNSUPPORTED in str(e), (kind, str(e))
            return True, extra
        return False, extra


def _same(a, b):
    if a is None or b is None:
        return a is b
    if isinstance(a, tuple):
        return all(_same(x, y) for x, y in zip(a, b))
    if isinstance(a, list):
        return M.state_bytes(a) == M.state_bytes(b)
    if isinstance(a, np.ndarray):
        return a.tobytes() == b.tobytes()
    return a == b


def _hold(tag, dev, model, before, after, out, kind):
    """the frame and the effect of one call, at every position"""
    from cerberus_amd import _ctypes as T
    first = {}
    for p, d in enumerate(dev.pos):
        w = model.w[d]
        for comp in M.COMPONENTS:
            got = after[comp][p]
            if d in first:
                assert _same(got, after[comp][first[d]]), (tag, comp, "positions", first[d], p, "of one window differ")
            if comp not in out.changed:
                assert _same(got, before[comp][p]), (tag, comp, "position", p, "changed by a call that leaves it alone")
            elif comp in out.exact:
                want = out.exact[comp][d]
                g = got[0] if comp == "records" else got
                assert _same(g, want), (tag, comp, "position", p, "is not the model's, bit for bit")
            elif comp in out.approx:
                want, err, bound, where = out.approx[comp]
                g = T.SolveSummary.from_buffer_copy(got) if comp == "summaries" else got
                e = err(g, want[d], w)
                assert e <= bound, (tag, comp, "position", p, e, bound, where)
        first.setdefault(d, p)
    for comp in set(out.approx) | out.adopt:
        vals = [after[comp][first[d]] for d in range(len(model.w))]
        if comp == "summaries":
            vals = [T.SolveSummary.from_buffer_copy(v) for v in vals]
        if comp == "records":
            vals = [v[0] for v in vals]
        model.adopt(comp, vals)


def make_model(ctx, cfg, ocfg, distinct):
    def pre(w, k, lin):
        a, b = int(w.sample_offsets[k]), int(w.sample_offsets[k + 1])
        off = np.array([0, b - a], np.int32)
        return (ctx.preintegrate(w.samples[a:b], off, lin[None]) if w.use_leg else ctx.preintegrate_imu(w.samples[a:b], off, lin[None, :6]))[0]
    return M.BatchModel(cfg, ocfg, distinct, pose_plus=ctx.pose_plus, preintegrate=pre)


class Runner:
    """One batch and its model, stepped through a sequence one call at a time (so that two batches can alternate)."""

    def __init__(self, ctx, cfg, ocfg, distinct, W, name, observed=True):
        self.name, self.dev, self.model = name, Device(ctx, distinct, W), make_model(ctx, cfg, ocfg, distinct)
        self.which, self.observed = "leg" if distinct[0].use_leg else "imu", observed
        self.k, self.seen, self.bytes = 0, set(), None
        self.obs = self.dev.observe(False)
        first = {d: p for p, d in reversed(list(enumerate(self.dev.pos)))}
        self.model.adopt_uploaded_records([self.obs["records"][first[d]][0] for d in range(len(distinct))])
        self.bytes = self.dev.b.device_bytes()[1]
        self.ops = list(M.SEQUENCES[name]) + [("solve", {})]   # the solve that ends the sequence

    def done(self):
        return self.k >= len(self.ops)

    def step(self):
        op = self.ops[self.k]
        tag = "%s[%d] %s" % (self.name, self.k, op[0])
        inputs = M.inputs_of(self.name, self.k, op, self.model.w)
        last = self.k == len(self.ops) - 1
        had_solved = self.dev.solves > 0
        if not self.observed and last:
            self.obs = self.dev.observe(self.model.snapshot is not None)   # (what the fresh batch is created from)
        fresh = self._fresh() if last else None
        self.dev.samples_on, self.dev.mask_now = self.model.samples_on, self.dev.per_position(self.model.mask)
        refused, extra = self.dev.run(op, inputs)
        out = self.model.apply((op[0], dict(op[1], **extra)), inputs)
        assert refused == out.refused, (tag, "refused" if refused else "went through", "the model says otherwise")
        if op[0] == "solve" and not refused and had_solved:
            assert self.dev.b.path()["replay"], tag
        if not self.observed and not last:
            self.k += 1
            return
        if last and (self.name, self.which) in M.ORACLE_REJECTS_END or not self.observed:
            out = out._replace(approx={}, adopt=set(out.approx) | out.adopt)   # (no oracle comparison: the frame and the fresh batch hold)
        after = self.dev.observe(self.model.snapshot is not None)
        if self.observed:
            _hold(tag, self.dev, self.model, self.obs, after, out, op[0])
            if op[0] == "marginalize" and not refused:
                zero = bytes(len(after["summaries"][0]))
                for p, w in enumerate(self.dev.ws):   # the header: the summaries are not kept (a window that is left alone may keep its own)
                    assert after["summaries"][p] == zero or (w.F != 11 and after["summaries"][p] == self.obs["summaries"][p]), (tag, "summaries", p)
                    assert w.F != 11 or after["summaries"][p] == zero, (tag, "summaries of a marginalised window", p)
        now = self.dev.b.device_bytes()[1]
        # Held against the figure after the previous call, which is the figure after the kind's first call unless another kind's first call
        # has grown it since (nothing ever shrinks it). A kind counts as new once more after the first save_state: the observation's
        # restore_state starts with it, and the calls' scratch is taken beside the snapshot from then on.
        kind = op[0] + ("" if self.model.snapshot is None else "+snapshot")
        if kind in self.seen and self.observed:
            assert now == self.bytes, (tag, "device bytes", self.bytes, now)
        self.seen.add(kind)
        self.bytes, self.obs = now, after
        if last:
            fresh.b.solve(fresh.opts)
            assert not fresh.b.path()["replay"]
            fs = fresh.b.download()
            assert [bytes(s) for s in fs] == after["summaries"], (tag, "summaries of the used and of a fresh batch differ")
            for p, w in enumerate(fresh.ws):
                assert M.state_bytes(M.trim(w, w.state_arrays())) == M.state_bytes(after["state"][p]), (tag, "position", p, "used and fresh batch differ")
            fresh.close()
        self.k += 1

    def _fresh(self):
        """a batch created from the downloaded state, the fetched records and the mask, samples in force if they are"""
        dev = self.dev
        ws = []
        for p, w in enumerate(dev.ws):
            t = w.twin()
            if w.use_leg:
                t.preint = w.preint.copy(); t.preint[:w.F - 1] = self.obs["records"][p][0]
            else:
                t.preint_imu = w.preint_imu.copy(); t.preint_imu[:w.F - 1] = self.obs["records"][p][0]
            ws.append(t)
        f = Device(dev.ctx, ws, len(ws), pos=list(range(len(ws))))
        mask = np.concatenate(self.obs["mask"]) if dev.off[-1] else np.zeros(0, np.uint8)
        if mask.any():
            f.b.mask_landmarks(mask=mask)
        if self.model.samples_on:
            f.b.set_samples(True)
        return f

    def close(self):
        self.dev.close()


def run_sequence(ctx, cfg, ocfg, distinct, W, name, observed=True):
    r = Runner(ctx, cfg, ocfg, distinct, W, name, observed)
    try:
        while not r.done():
            r.step()
    finally:
        r.close()
    return r


class _Form:
    def __init__(self, ctx, form):
        self.ctx, self.form = ctx, form

    def __enter__(self):
        self.ctx.set_solver_form(self.form)

    def __exit__(self, *a):
        self.ctx.set_solver_form("auto")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("which", ["leg", "imu"])
@pytest.mark.parametrize("name", list(M.SEQUENCES))
def test_sequence(ctx, cfg, ocfg, sets, name, which, form):
    with _Form(ctx, form):
        run_sequence(ctx, cfg, ocfg, sets[which], SIZES[which], name)


UNOBSERVED = ("trial_step", "samples_roundtrip", "startup_then_steady", "writebacks", "mask_cycle")


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("name", UNOBSERVED)
def test_sequence_without_observation(ctx, cfg, ocfg, sets, name, form):
    """The observation puts reset, restore_state, a set_state of every window and a zero OR round between any two calls: no pair is adjacent
    on the device, every state a call reads was last written by k_set_state, and the mask call may drop captures. Here the calls run back to
    back, held only by their refusals, the replay flag of every later solve, marginalize's priors and, before and after the closing solve,
    the comparison with a fresh batch (bit for bit)."""
    with _Form(ctx, form):
        r = run_sequence(ctx, cfg, ocfg, sets["leg"], SIZES["leg"], name, observed=False)
        if any(k == "marginalize" for k, _ in M.SEQUENCES[name]):
            assert r.dev.priors_held > 0


def test_priors_were_held(ctx, cfg, ocfg, sets):
    """marginalize after an OR round of the outlier flags (startup_then_steady) and after a mask and an OR round (masked_refusals): the
    priors were compared for every 11-frame window, each at four positions"""
    for name in ("startup_then_steady", "masked_refusals"):
        r = run_sequence(ctx, cfg, ocfg, sets["leg"], SIZES["leg"], name)
        assert r.dev.priors_held >= 4 * sum(1 for w in sets["leg"] if w.F == 11), (name, r.dev.priors_held)


@pytest.mark.parametrize("form", FORMS)
def test_two_batches_alternate(ctx, cfg, ocfg, sets, form):
    """Two batches of one context run trial_step and writebacks with their calls alternating (arena chunks of one go back to the
    context's pool while the other holds its own): each is held against its model call by call, and ends bit for bit where it ends alone."""
    with _Form(ctx, form):
        alone = {}
        for name in M.TWO_BATCHES:
            r = run_sequence(ctx, cfg, ocfg, sets["leg"], SIZES["leg"], name)
            alone[name] = ([M.state_bytes(s) for s in r.obs["state"]], r.obs["summaries"])
        rs = [Runner(ctx, cfg, ocfg, sets["leg"], SIZES["leg"], name) for name in M.TWO_BATCHES]
        try:
            while not all(r.done() for r in rs):
                for r in rs:
                    if not r.done():
                        r.step()
            for r in rs:
                assert ([M.state_bytes(s) for s in r.obs["state"]], r.obs["summaries"]) == alone[r.name], r.name
        finally:
            for r in rs:
                r.close()


def test_row_G_environment():
    """Every sequence on the leg batch once more in a child under row G's switches (pc visual form, paired IMU, two-kernel assembly, split
    solver: the benchmark's kernel set, at 32 windows)."""
    from test_kernel_paths import _G
    env = {k: v for k, v in os.environ.items() if not k.startswith("VILO_") or k == "VILO_GPU_LIB"}
    env.update(_G)
    p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "_sequences_worker.py")], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    line = next((l for l in p.stdout.splitlines() if l.startswith("SEQUENCES_JSON ")), None)
    assert p.returncode == 0 and line, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    res = json.loads(line[len("SEQUENCES_JSON "):])
    assert set(res["results"]) == set(M.SEQUENCES) and res["path"]["solver"] == "split" and res["path"]["imu"] == "pair", res["path"]
    bad = {n: r for n, r in res["results"].items() if r != "ok"}
    assert not bad, bad
