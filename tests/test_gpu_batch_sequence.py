"""History independence of a staged batch: ONE Batch and ONE Context driven through the generated sequences of
tests/batch_sequence.py, every observable result of every step compared bit for bit with the model — return codes, verdicts,
statuses, accumulator bytes, failed counts and indices, summary words, re-check and identify results, exported records (as affine
points: identical launches differ in Jacobian form), a fresh accumulator fed the batch, the one-shot calls of the same context and a
second batch in flight.  The expected values are batch_sequence.Expect's: the references only, never the library.

tests/test_batch_sequence_host.py holds the committed cases to what they must cover.  A mismatch fails with the trace up to the step
(each line replays on the driver: `run.upload(...)`) and one diagnosis: the step's own upload -> launch -> read on a fresh Batch,
and whether THAT agrees with the reference — if it does, the bug depends on the history."""
import collections
import random

import pytest

import batch_sequence as bs
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu

PLEN = 1024
ZERO = bytes(64)
POISON = -286331154          # 0xEEEEEEEE as int32: no launch writes it
ERR_DEVICE = -18
ACC_BYTES = 1312             # include/h2v.h H2V_ACC_RECORD_BYTES


@pytest.fixture(scope="module")
def world():
    """the key, 96 + 3 x 16 proofs, ONE context for the whole module, and the references' caches"""
    import halo2_verifier_amd as h2v
    s = circuits.setup_vector_mul(8, 8)
    pools = {8: circuits.prove_vector_mul_batch(s, 96, seed=4242, threads=16)}
    rnd = random.Random(77)
    for m in (5, 3, 0):
        P, I = [], []
        for j in range(16):
            a = [rnd.randrange(R_MOD) for _ in range(s.n_mul)]
            b = [rnd.randrange(R_MOD) for _ in range(m)] + [0] * (s.n_mul - m)
            p, inst = circuits.prove_vector_mul_len(s, a, b, m, rng_seed=4000 + 100 * m + j)
            P.append(p); I.append(inst)
        pools[m] = (P, I)
    assert all(len(p) == PLEN for P, _ in pools.values() for p in P)
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    yield ctx, bs.Expect(s, pools), pools
    ctx.close()
    s.free()


def _flat(P, I):
    return b"".join(P), b"".join(b"".join(col) for i in I for col in i)


def _rand_bytes(rand):
    return b"".join(int(r).to_bytes(32, "little") for r in rand)


class Mismatch(AssertionError):
    pass


class Driver:
    """Plays steps on one Batch: every method is an operation of batch_sequence's alphabet, so a trace line replays as `run.<op>(...)`."""

    def __init__(self, ctx, expect, pools, diagnose=True, capacity=bs.CAPACITY):
        import halo2_verifier_amd as h2v
        self.h2v, self.ctx, self.expect, self.pools, self.diagnose, self.capacity = h2v, ctx, expect, pools, diagnose, capacity
        self.b = h2v.Batch(ctx, capacity, 8)
        self.b2 = None
        self.model = bs.Model(capacity)
        self.done = []                       # the steps so far
        self.reached = collections.Counter()
        self.statuses_seen = set()
        self.dead = False                    # a HIP error: nothing more is started

    def close(self):
        for b in (self.b, self.b2):
            if b is not None:
                b.close()

    def play(self, steps):
        for s in steps:
            self.step(s)

    def __getattr__(self, op):               # run.upload(route=...): the trace's lines
        if op.startswith("_") or op not in ("set_groups", "set_group_sizes", "upload", "launch", "illegal", "ctx_call", "second_start", "second_finish") + bs.READERS:
            raise AttributeError(op)
        return lambda **kw: self.step(bs.Step(op, **kw))

    # ------------------------------------------------------------------ one step
    def step(self, s):
        assert not self.dead, "a HIP error ended this sequence"
        before = self.model.view()
        out = self.model.apply(s)
        self.done.append(s)
        try:
            if out.kind == "ok":
                getattr(self, "_" + s.op)(out.view, **s.kw)
            else:
                try:
                    getattr(self, "_" + s.op)(out.view, **s.kw)
                except self.h2v.H2VError as e:
                    if e.code == ERR_DEVICE:
                        raise
                    self.same("the refusal's code", e.code, out.code)
                else:
                    raise Mismatch(f"the call succeeded; the model says it is refused with {out.code}")
                self.reached[out.kind] += 1
                if s.op == "upload":
                    self.reached["upload refused: " + s.kw["route"]] += 1
                elif out.kind == "refused_empty":
                    self.reached["deferred draw fault refused"] += 1
        except self.h2v.H2VError as e:
            if e.code == ERR_DEVICE:
                self.dead = True             # never expected: stop here and start nothing more
                pytest.fail(f"HIP error at step {len(self.done)}: {e}\n{bs.trace(self.done)}", pytrace=False)
            self.fail(s, before, f"unexpected {e}")
        except Mismatch as e:
            self.fail(s, before, str(e))

    def same(self, what, got, want):
        if got != want:
            raise Mismatch(f"{what}: got {self.short(got)}, the reference says {self.short(want)}")

    @staticmethod
    def short(v):
        text = repr(v)
        return text if len(text) < 600 else text[:300] + " ... " + text[-300:]

    def fail(self, s, before, why):
        note = ""
        if self.diagnose and before.up is not None and s.op in bs.READERS:
            note = "\nfresh batch: " + self.fresh_replay(s, before)
        pytest.fail(f"step {len(self.done)} ({s.line()}): {why}{note}\ntrace:\n{bs.trace(self.done)}", pytrace=False)

    def fresh_replay(self, s, view):
        """the step's own upload -> launch -> read on a fresh Batch of the same context"""
        steps = []
        if view.sizes is not None:
            steps.append(bs.Step("set_group_sizes", sizes=view.sizes))
        elif view.groups != 1:
            steps.append(bs.Step("set_groups", groups=view.groups))
        steps.append(bs.Step("upload", **view.up))
        if view.up["route"] != "upload_launch":
            steps.append(bs.Step("launch", pairing=bool(view.pairing)))
        if bs.LEAST[s.op] == bs.FINISHED and view.fault is None:
            steps.append(bs.Step("finish_groups"))
        steps.append(s)
        fresh = Driver(self.ctx, self.expect, self.pools, diagnose=False, capacity=self.capacity)
        try:
            fresh.play(steps)
            return "the same upload, launch and read on a fresh Batch AGREE with the reference: the failure depends on the history"
        except BaseException as e:   # (pytest.fail raises outside Exception)
            return f"a fresh Batch disagrees with the reference as well ({str(e).splitlines()[0]}): not a matter of history"
        finally:
            fresh.close()

    # ------------------------------------------------------------------ configure, upload, launch
    def _set_groups(self, view, groups):
        self.b.set_groups(groups)

    def _set_group_sizes(self, view, sizes):
        self.b.set_group_sizes(sizes)

    def upload_into(self, batch, up, groups, sizes):
        import torch
        P, I = bs.materialise(up, groups, sizes, self.pools)
        flat, inst = _flat(P, I)
        draws = bs.draws_of(up)
        cols, n = [up["shape"]], up["n"]
        if up["route"] == "upload":
            batch.upload(flat, PLEN, inst, cols, _rand_bytes(draws))
        elif up["route"] == "upload_launch":
            batch.upload_launch(flat, PLEN, inst, cols, _rand_bytes(draws), with_pairing=up["pairing"])
        else:
            proofs = torch.frombuffer(bytearray(flat), dtype=torch.uint8).reshape(n, PLEN).cuda()
            insts = torch.frombuffer(bytearray(inst), dtype=torch.uint8).reshape(n, 32 * up["shape"]).cuda() if up["shape"] else None
            tail = torch.frombuffer(bytearray(_rand_bytes(draws)), dtype=torch.uint8).reshape(n, 32).cuda() if draws is not None else None
            batch.upload_tensors(proofs, insts, cols, tail)

    def _upload(self, view, **up):
        self.upload_into(self.b, up, self.model.groups, self.model.sizes)

    def _launch(self, view, pairing):
        self.b.launch(with_pairing=pairing)

    # ------------------------------------------------------------------ the readers
    def note(self, view, oks, statuses, lefts, rights):
        """what a case was designed to reach, seen in a result that has just been compared with the reference"""
        self.statuses_seen |= {v for v in statuses if v}
        if lefts is not None and ZERO in lefts and not any(statuses):
            self.reached["identity accumulator"] += 1
        if not any(statuses) and not all(oks):
            self.reached["rejected by the pairing alone"] += 1
        if any(statuses):
            self.reached["rejected by a status"] += 1
        if all(oks):
            self.reached["accepted"] += 1

    def compare_finish(self, view, got, single):
        oks, st, lefts, rights = self.expect.finish_groups(view)
        if single:
            got = ([got[0]], got[1], [got[2]], [got[3]])
        self.same("group_ok", list(got[0]), oks)
        self.same("statuses", got[1], st)
        if lefts is not None:
            self.same("left accumulators", got[2], lefts)
            self.same("right accumulators", got[3], rights)
        else:   # OS draws: the points are the library's own; an accumulator is the identity exactly when its group has no accepted proof
            off = self.expect.launch(view)["off"]
            empty = [all(st[a:b]) for a, b in zip(off, off[1:])]
            self.same("left accumulators that are the identity", [p == ZERO for p in got[2]], empty)
            self.same("right accumulators that are the identity", [p == ZERO for p in got[3]], empty)
        self.note(view, oks, st, lefts, rights)

    def _finish(self, view):
        self.compare_finish(view, self.b.finish(), True)

    def _finish_groups(self, view):
        self.compare_finish(view, self.b.finish_groups(), False)

    def _finish_into(self, view, outputs, cap):
        import torch
        n, G = self.b.n, self.b.groups
        full = lambda count, dtype: torch.full((count,), 0xEE if dtype == torch.uint8 else POISON, dtype=dtype, device="cuda:0")
        t = {"status": full(n, torch.int32), "group_ok": full(G, torch.int32), "left_xy": full(64 * G, torch.uint8).reshape(G, 64),
             "right_xy": full(64 * G, torch.uint8).reshape(G, 64), "group_failed": full(G, torch.int32), "failed_index": full(n if cap is None else cap, torch.int32),
             "summary": full(8, torch.int32)}
        self.b.finish_into(**{k: t[k] for k in outputs})
        torch.cuda.synchronize()
        if self.model.stage < bs.LAUNCHED:
            return                            # (an illegal call that was not refused: the caller reports it)
        want = self.expect.finish_into(view, cap)
        points = lambda k: [bytes(t[k][g].cpu().numpy().tobytes()) for g in range(G)]
        for k in outputs:
            if k in ("left_xy", "right_xy"):
                if want[k] is not None:
                    self.same(k, points(k), want[k])
            elif k == "failed_index":
                got = [v & 0xffffffff for v in t[k].tolist()]
                idx = want[k][:len(got)]
                self.same(k, got, idx + [0xEEEEEEEE] * (len(got) - len(idx)))
            elif k in ("summary", "group_failed"):
                self.same(k, [v & 0xffffffff for v in t[k].tolist()], want[k])
            else:
                self.same(k, t[k].tolist(), want[k])
        for k in bs.OUTPUTS:                  # an output not asked for is not written
            if k not in outputs:
                self.same(k + " (not given)", set(t[k].flatten().tolist()) <= {POISON, 0xEE}, True)
        if view.fault is not None and "summary" in outputs:
            self.reached["deferred draw fault in the summary"] += 1

    def _recheck(self, view, ranges):
        got = self.b.recheck(ranges)
        oks, lefts, rights = self.expect.recheck(view, ranges)
        self.same("recheck verdicts", got[0], oks)
        if lefts is not None:
            self.same("recheck left", got[1], lefts)
            self.same("recheck right", got[2], rights)

    def _identify(self, view):
        st, own, _ = self.b.identify()
        want_st, want_own = self.expect.identify(view)
        self.same("identify statuses", st, want_st)
        self.same("identify group_own_ok", own, want_own)
        if any(v == self.h2v.PlonkError.ConstraintSystemFailure for v in st):
            self.reached["identify named a proof"] += 1

    def _export(self, view):
        import numpy as np
        import torch
        import msm_reference as ref
        import record_reference
        G = self.b.groups
        rec = torch.zeros(G * ACC_BYTES, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        self.b.export_accumulators(rec.data_ptr())
        torch.cuda.synchronize()
        if self.model.stage < bs.LAUNCHED or self.model.sizes is not None:
            return
        words = np.frombuffer(bytes(rec.cpu().numpy().tobytes()), dtype="<u4").tolist()
        for g, (failed, left, right) in enumerate(self.expect.export(view)):
            w = words[g * (ACC_BYTES // 4):(g + 1) * (ACC_BYTES // 4)]
            self.same(f"record {g}: failed and the reserved word", [w[0], w[3]], [failed, 0])
            self.same(f"record {g}: a piece count in 1 .. 6", 1 <= w[1] <= record_reference.PIECES, True)
            if bs.draws_of(view.up) is None:
                continue
            for side, want in ((0, left), (1, right)):
                pieces = [ref.jac_point(w[4 + 27 * (6 * side + j):31 + 27 * (6 * side + j)]) for j in range(w[1])]
                self.same(f"record {g} side {side}", record_reference.weighted_sum(pieces, w[2]), want)

    def _process_batch(self, view):
        acc = self.h2v.Accumulator(self.ctx)
        try:
            added = acc.process_batch(self.b)
            read, final = acc.read(), acc.finalize()
        finally:
            acc.close()
        want_added, want_read, want_final = self.expect.process_batch(view)
        self.same("process_batch counters", added, want_added)
        self.same("accumulator counters", read[2:], want_read[2:])
        self.same("accumulator verdict", final[0], want_final[0])
        if want_read[0] is not None:
            self.same("accumulator points", read[:2], want_read[:2])
            self.same("finalize points", final[1:], want_final[1:])

    # ------------------------------------------------------------------ calls the stage refuses
    def _illegal(self, view, call):
        if call in ("finish", "finish_grouped"):
            self.b.finish()
        elif call == "finish_groups":
            self.b.finish_groups()
        elif call == "launch":
            self.b.launch()
        elif call == "finish_into":
            self._finish_into(view, ["summary"], None)
        elif call in ("export", "export_ragged"):
            self._export(view)
        elif call == "identify" or call == "identify_zero":
            self.b.identify()
        elif call == "process_batch":
            self._process_batch(view)
        elif call == "recheck":
            self.b.recheck([(0, 1)])
        elif call == "recheck_cross":
            off = bs.group_offsets(view.up["n"], view.groups, view.sizes)
            self.b.recheck([(off[1] - 1, 2)])
        elif call == "recheck_zero":
            off, zero = bs.group_offsets(view.up["n"], view.groups, view.sizes), bs.zero_below(view.up, view.groups, view.sizes)
            g = next(k for k, z in enumerate(zero) if z)
            self.b.recheck([(off[g] + zero[g] - 1, 2 if off[g] + zero[g] < off[g + 1] else 1)])
        else:
            raise ValueError(call)

    # ------------------------------------------------------------------ the same context beside the batch
    def _ctx_call(self, view, kind, shape, seed):
        args = self.expect.ctx_inputs(kind, shape, seed)
        want = self.expect.ctx_call(kind, shape, seed)
        if kind == "verify_batch":
            got = self.ctx.verify_batch(*args)
        elif kind == "verify_each":
            got = self.ctx.verify_each(args[0], args[1])
        elif kind == "verify_batch_identify":
            got = self.ctx.verify_batch_identify(*args)
        elif kind == "guard_msm":
            got = self.ctx.guard_msm(*args)
        elif kind == "msm_g1":
            got = self.ctx.msm_g1(*args)
        else:
            msms = [self.h2v.MSMKZG(self.ctx) for _ in args]
            try:
                for m, (sc, bases) in zip(msms, args):
                    m.append_terms(sc, bases)
                got, ident = self.h2v.eval_many(msms)
                self.same("eval_many identity flags", ident, [p == ZERO for p in want])
            finally:
                for m in msms:
                    m.close()
        self.same(kind, got, want)
        self.reached["ctx " + kind] += 1

    def _second_start(self, view, n, shape, groups, content, seed):
        if self.b2 is None:
            self.b2 = self.h2v.Batch(self.ctx, 128, 8)
        self.b2.set_groups(groups)
        up = bs.second_upload(dict(n=n, shape=shape, content=content, seed=seed))
        self.upload_into(self.b2, up, groups, None)
        self.b2.launch()

    def _second_finish(self, view):
        got = self.b2.finish_groups()
        oks, st, lefts, rights = self.expect.finish_groups(view)
        self.same("the second batch", got, (oks, st, lefts, rights))
        self.reached["second batch finished"] += 1


def _designed(steps, capacity):
    """what the sequence was made to reach, from its own steps: the driver must have seen it (a wrong model cannot make the test vacuous)"""
    want = collections.Counter()
    for s, before, out in bs.run_model(steps, capacity):
        if out.kind != "ok":
            want[out.kind] += 1
        if s.op in ("finish", "finish_groups") and out.kind == "ok" and out.view.up["route"] != "device_os":
            up = out.view.up
            even = all(sz % 2 == 0 for sz in bs.group_sizes(up["n"], out.view.groups, out.view.sizes))
            if up["draws"] == "alternating" and up["content"] == "clean" and even:
                want["identity accumulator"] += 1
            if up["content"] in ("point", "eval", "two"):
                want["rejected by a status"] += 1
            if up["content"] in ("input", "sign") and up["draws"] == "random" and out.view.pairing:
                want["rejected by the pairing alone"] += 1
        if s.op == "ctx_call":
            want["ctx " + s.kw["kind"]] += 1
        if s.op == "second_finish":
            want["second batch finished"] += 1
    return want


def _check_reached(run, steps):
    want = _designed(steps, run.capacity)
    for what, count in want.items():
        assert run.reached[what] >= count, (what, run.reached[what], count)
    return want


@pytest.mark.parametrize("case", range(len(bs.CASES)), ids=["%d-%s" % c[:2] for c in bs.CASES])
def test_one_batch_through_a_generated_sequence(world, case):
    ctx, expect, pools = world
    seed, focus, n_steps = bs.CASES[case]
    steps = bs.sequence(seed, n_steps, focus)
    run = Driver(ctx, expect, pools)
    try:
        run.play(steps)
        _check_reached(run, steps)
    finally:
        run.close()


def test_one_large_batch_across_the_overlapped_upload(world):
    """2048 proofs a launch, where h2v_batch_upload_launch decompresses under its copy: every other route directly behind such an upload"""
    ctx, expect, pools = world
    steps = bs.large_sequence()
    run = Driver(ctx, expect, pools, capacity=bs.LARGE_CAPACITY)
    try:
        run.play(steps)
        assert _check_reached(run, steps)["rejected by a status"] >= 3 and len(run.statuses_seen) >= 2
    finally:
        run.close()


def test_one_batch_through_every_sequence(world):
    """all cases back to back on ONE Batch (and the module's one Context), in a fixed shuffled order"""
    ctx, expect, pools = world
    run = Driver(ctx, expect, pools)
    try:
        for k in bs.SHUFFLED:
            seed, focus, n_steps = bs.CASES[k]
            seq = bs.sequence(seed, n_steps, focus)
            if run.model.second is not None:      # (the case before left its second batch in flight)
                seq = [bs.Step("second_finish")] + seq
            run.play([bs.Step("set_groups", groups=1)] + seq)   # a sequence starts from one group; everything else is as the case before left it
        # together the cases reach every kind of result the alphabet can produce
        assert run.reached["identity accumulator"] >= 1 and run.reached["rejected by the pairing alone"] >= 1 and run.reached["accepted"] >= 1
        assert len(run.statuses_seen) >= 2, run.statuses_seen
        assert run.reached["upload refused: upload"] >= 1 and run.reached["upload refused: upload_launch"] >= 1 and run.reached["deferred draw fault refused"] >= 1
        assert run.reached["deferred draw fault in the summary"] >= 1 and run.reached["identify named a proof"] >= 1
        assert all(run.reached["ctx " + kind] >= 1 for kind in bs.CTX_KINDS) and run.reached["second batch finished"] >= 1
    finally:
        run.close()
