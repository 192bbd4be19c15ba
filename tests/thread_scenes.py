"""Scenes for the threading contract of include/h2v.h (host only: nothing here touches the GPU library).

A context may be shared between host threads; a batch, an accumulator or an MSM object is used by one thread at a time, many of them
in flight on one context.  A scene is a fixed schedule: per repetition the contexts and objects to create, per thread a list of calls
whose arguments are complete before the start, a start barrier, and the expected result of every call.  The expected values come only
from the references the suite already has — batch_reference (linearity over the oracle's per-proof Guards), circuits.oracle_*,
results_reference, oracle_lib.g1_msm — never from a run of the library.  Every thread has its own proofs, draws and defects, so a
result delivered to the wrong thread is a mismatch.

    build(seed) -> {"keys": {name: (params, vk)}, "scenes": [scene]}
    scene = {"name", "reps": [rep]};  rep = {"contexts": [(name, key or None)], "objects": [(name, kind, context, init)],
                                            "threads": [[call]], "main_after": [call], "barrier_rounds": bool}
    call  = {"op", "on", "uses", "args", "expect", "error", "after", "round"}

`uses` names the objects the call needs for itself; `after` names the call (thread, index) whose return it waits for, which is how an
object changes hands; `round` makes the thread wait at the scene's barrier before the call.  tests/thread_driver.py plays a scene,
tests/test_gpu_threads.py compares, tests/test_thread_scenes_host.py holds the schedules to what they must cover."""
import random

import batch_reference
import circuits
import oracle_lib
import results_reference as rr
from circuits import R_MOD, le32

ZERO = bytes(64)
ANY = "*"                      # in an expectation: whatever the library returns here (the points under OS draws)
BAD_ARGUMENT, UNSUPPORTED, ERR_DEVICE = -16, -19, -18
MAX_THREADS = 8
MAX_CACHED_PLANS = 32          # csrc/vkplan.h H2V_MAX_CACHED_PLANS
DEFECTS = ("clean", "tamper", "input", "noncanon")     # (+ a zero draw, which is a property of the draws)

# what every op of the alphabet calls in the C library (through halo2_verifier_amd/verifier.py and distributed.py)
OP_SYMBOLS = {
    "verify_batch": ("h2v_verify_batch",), "verify_batch_seeded": ("h2v_verify_batch_seeded",), "verify_batch_shapes": ("h2v_verify_batch_shapes",),
    "verify_batch_identify": ("h2v_verify_batch_identify",), "verify_batches": ("h2v_verify_batches",), "verify_each": ("h2v_verify_each",),
    "verify_batch_keys": ("h2v_verify_batch_keys",), "guard_msm": ("h2v_guard_msm",), "guards_check_each": ("h2v_guards_check_each",),
    "msm_g1": ("h2v_msm_g1",), "pairing_check": ("h2v_pairing_check",),
    "msm_append": ("h2v_msm_append_terms",), "msm_scale": ("h2v_msm_scale",), "msm_scalars": ("h2v_msm_len", "h2v_msm_terms"),
    "msm_add_msm": ("h2v_msm_add_msm",), "msm_eval_many": ("h2v_msm_eval_many",), "dual_check_many": ("h2v_dual_msm_check_many",),
    "b_set_groups": ("h2v_batch_set_groups",), "b_set_group_sizes": ("h2v_batch_set_group_sizes",), "b_upload": ("h2v_batch_upload",),
    "b_launch": ("h2v_batch_launch",), "b_upload_launch": ("h2v_batch_upload_launch",), "b_finish": ("h2v_batch_finish",),
    "b_finish_groups": ("h2v_batch_finish_groups",), "b_upload_tensors": ("h2v_batch_stream", "h2v_batch_upload_device"),
    "b_finish_into": ("h2v_batch_stream", "h2v_batch_finish_device"), "b_recheck": ("h2v_batch_recheck",), "b_identify": ("h2v_batch_identify",),
    "a_process": ("h2v_accumulator_process",), "a_process_guards": ("h2v_accumulator_process_guards",),
    "a_process_batch": ("h2v_accumulator_process_batch",), "a_add_msm": ("h2v_accumulator_add_msm",), "a_read": ("h2v_accumulator_read",),
    "a_finalize": ("h2v_accumulator_finalize",), "a_merge": ("h2v_accumulator_merge",), "a_export_state": ("h2v_accumulator_export_state",),
    "verify_batch_seeded_identify": ("h2v_verify_batch_seeded_identify",), "verify_batch_keys_identify": ("h2v_verify_batch_keys_identify",),
    "a_add_msms": ("h2v_accumulator_add_msms",), "b_recheck_many": ("h2v_batches_recheck",), "b_accumulators": ("h2v_batch_accumulators",),
    "b_export": ("h2v_batch_export_accumulators",), "fold_check": ("h2v_fold_check",), "b_fold_enqueue": ("h2v_batch_fold_check_enqueue",),
    "b_set_stream": ("h2v_batch_set_stream",), "b_stream": ("h2v_batch_stream",), "a_journal_begin": ("h2v_accumulator_journal_begin",), "a_check_legs": ("h2v_accumulator_check_legs",),
    "a_drop_legs": ("h2v_accumulator_drop_legs",), "a_merge_states": ("h2v_accumulator_merge_states",),
    "merge_local": ("h2v_accumulator_export_state", "h2v_accumulator_journal_begin", "h2v_accumulator_merge_states", "h2v_accumulator_finalize",
                    "h2v_accumulator_check_legs"),
}
ERROR_SYMBOLS = ("h2v_last_error",)       # every refusal reads its text

# Symbols no scene has to enter from two threads at once: symbol -> reason.  tests/test_thread_scenes_host.py holds this list and the
# scenes' reach to _lib.SIGNATURES: a new entry point must be put into a scene or excluded here.
HOST_ONLY = "a host-only converter or probe: no context, no device state"
OWNER = "create / destroy of an object by its owner"
EXCLUDED = {
    "h2v_device_count": HOST_ONLY, "h2v_abi_version": HOST_ONLY, "h2v_vk_convert": HOST_ONLY, "h2v_params_convert": HOST_ONLY,
    "h2v_random_scalars": HOST_ONLY, "h2v_ctx_proof_shape": HOST_ONLY,
    "h2v_last_error": "host only: returns the calling thread's own text (the errors scene holds every text to its thread)",
    "h2v_msm_len": "host only: reads one field of the caller's own object",
    "h2v_ctx_create": OWNER, "h2v_ctx_create_ex": OWNER, "h2v_ctx_destroy": OWNER, "h2v_batch_create": OWNER, "h2v_batch_destroy": OWNER,
    "h2v_accumulator_create": OWNER, "h2v_accumulator_destroy": OWNER, "h2v_msm_create": OWNER, "h2v_msm_destroy": OWNER,
    "h2v_ctx_set_tuning": "documented as not synchronised with launches: set while the context is idle",
    "h2v_batch_set_profiling": "profiling: timing only, no result", "h2v_batch_timings": "profiling: timing only, no result",
}


# ------------------------------------------------------------------ plain data
def canon(v):
    """a result as JSON holds it: bytes as hex, tuples as lists"""
    if isinstance(v, (bytes, bytearray)):
        return bytes(v).hex()
    if isinstance(v, (list, tuple)):
        return [canon(x) for x in v]
    if isinstance(v, dict):
        return {str(k): canon(x) for k, x in sorted(v.items())}
    if v is None or isinstance(v, (bool, int, str)):
        return v
    raise TypeError(type(v))


def matches(got, want):
    """bit for bit, but for ANY"""
    if isinstance(want, str) and want == ANY:
        return True
    if isinstance(want, list):
        return isinstance(got, list) and len(got) == len(want) and all(matches(g, w) for g, w in zip(got, want))
    if isinstance(want, dict):
        return isinstance(got, dict) and sorted(got) == sorted(want) and all(matches(got[k], want[k]) for k in want)
    return type(got) is type(want) and got == want


def call(op, on=None, uses=(), expect=None, error=None, after=None, round=None, **args):
    assert op in OP_SYMBOLS, op
    return {"op": op, "on": on, "uses": list(uses), "args": args, "expect": canon(expect), "error": list(error) if error else None,
            "after": after, "round": round}


def spoil(proof, instances, kind):
    """clean; tamper: an evaluation's low bit (status 0, the pairing fails); input: a wrong public input (the same); noncanon: an
    evaluation that is no canonical scalar (status -5)"""
    if kind == "clean":
        return proof, instances
    if kind == "input":
        first = (int.from_bytes(instances[0][0], "little") + 1) % R_MOD
        return proof, [[le32(first)] + list(instances[0][1:])] + [list(c) for c in instances[1:]]
    b = bytearray(proof)
    if kind == "tamper":
        b[700] ^= 1
    elif kind == "noncanon":
        b[-96:-64] = b"\xff" * 32
    else:
        raise ValueError(kind)
    return bytes(b), instances


def flat(P, I):
    return b"".join(P), b"".join(b"".join(col) for i in I for col in i)


def draw_bytes(draws):
    return b"".join(le32(d) for d in draws)


def offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


# ------------------------------------------------------------------ the keys and the proofs
class World:
    """the three k = 8 vector_mul keys over one params, and every proof the scenes use (made once, by the CPU prover)"""

    def __init__(self, seed):
        self.seed = seed
        self.s8, self.s4, self.s70 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4), circuits.setup_vector_mul(8, 70)
        assert self.s8.params == self.s4.params == self.s70.params
        self.L = self.s8.L
        P, I = circuits.prove_vector_mul_batch(self.s8, 96, seed=seed, threads=8)
        self.pool8 = list(zip(P, I))
        P, I = circuits.prove_vector_mul_batch(self.s4, 24, seed=seed + 1, threads=8)
        self.pool4 = list(zip(P, I))
        rnd = random.Random(seed + 2)
        self.shapes = {}          # public inputs -> [(proof, instances)] x 6: one per plan-churn thread
        for m in range(1, 41):
            self.shapes[m] = []
            for j in range(6):
                a = [rnd.randrange(R_MOD) for _ in range(70)]
                b = [rnd.randrange(R_MOD) for _ in range(m)] + [0] * (70 - m)
                self.shapes[m].append(circuits.prove_vector_mul_len(self.s70, a, b, m, rng_seed=seed * 1000 + 10 * m + j))
        self.plen = len(self.pool8[0][0])
        assert all(len(p) == self.plen for p, _ in self.pool8 + self.pool4)
        self.keys = {"k8": (self.s8.params, self.s8.vk), "k4": (self.s4.params, self.s4.vk), "k70": (self.s70.params, self.s70.vk)}
        self._each, self._pairing = {}, {}

    def free(self):
        for s in (self.s8, self.s4, self.s70):
            s.free()

    def own(self, t, count=8):
        """thread t's own proofs of the 8-input key: no other thread of any scene's repetition has them"""
        return self.pool8[t * count:(t + 1) * count]

    def each(self, item):
        key = batch_reference._key(*item)
        if key not in self._each:
            self._each[key] = circuits.oracle_verify_single(*item)
        return self._each[key]

    def guard(self, item):
        rc, g = circuits.oracle_guard(*item)
        assert rc == 0
        return ((g["left_scalars"], g["left_bases"]), (g["right_scalars"], g["right_bases"]))

    def points(self, item):
        rc, L, R = batch_reference.single(*item)
        assert rc == 0
        return L, R

    def bases(self, item):
        """points on the curve: the right bases of the item's Guard"""
        return [b for b in self.guard(item)[1][1] if any(b)]

    def pairing(self, left, right):
        if (left, right) not in self._pairing:
            self._pairing[(left, right)] = circuits.oracle_pairing_check(self.s8, left, right)
        return self._pairing[(left, right)]

    def expected(self, items, draws, seed=None):
        """batch_reference.expected, its pairing remembered"""
        extra = ()
        if seed is not None:
            M = 1
            for d in draws:
                M = M * d % R_MOD
            extra = [(M, seed[0], seed[1])]
        st, left, right = batch_reference._accumulate(self.s8, items, batch_reference.multipliers(draws), extra)
        return (not any(st) and self.pairing(left, right)), st, left, right

    def msm(self, scalars, bases):
        terms = [(s % R_MOD, b) for s, b in zip(scalars, bases)]
        return oracle_lib.g1_msm(self.L, [s for s, _ in terms], [b for _, b in terms]) if terms else ZERO


class AccModel:
    """a resident accumulator, from the references: (L, R) = sum coef (L_i, R_i) over evaluated Guards"""

    def __init__(self, w):
        self.w, self.terms, self.n, self.failed = w, [], 0, 0

    def process(self, items, draws, guards=False):
        M = 1
        for d in draws:
            M = M * d % R_MOD
        for t in self.terms:
            t[0] = t[0] * M % R_MOD
        st = []
        for it, m in zip(items, batch_reference.multipliers(draws)):
            rc, L, R = batch_reference.single(*it)
            st.append(rc)
            if rc == 0:
                self.terms.append([m, L, R])
        assert not (guards and any(st))
        self.n += len(items)
        self.failed += sum(1 for v in st if v)
        return st

    def add(self, left, right):
        self.terms.append([1, left, right])

    def read(self):
        cl, cr = {}, {}
        for c, L, R in self.terms:
            cl[L] = cl.get(L, 0) + c
            cr[R] = cr.get(R, 0) + c
        return batch_reference._combine(self.w.s8, cl), batch_reference._combine(self.w.s8, cr), self.n, self.failed

    def finalize(self):
        left, right, _, failed = self.read()
        return (not failed and self.w.pairing(left, right)), left, right


def launch_expect(w, items, draws, sizes, pairing=True):
    """a grouped launch -> (group_ok, statuses, lefts, rights, own pairing bits) as Batch.finish_groups returns the first four"""
    off = offsets(sizes)
    oks, st, lefts, rights, pair = [], [], [], [], []
    for a, b in zip(off, off[1:]):
        _, s, left, right = w.expected(items[a:b], draws[a:b])
        p = w.pairing(left, right)
        oks.append(not any(s) and (p or not pairing)); st += s; lefts.append(left); rights.append(right); pair.append(p)
    return oks, st, lefts, rights, pair


def pick(w, rnd, pool, key, n, defect="clean", at=None):
    """n items of the thread's pool (with repeats), one of them spoiled -> (items, proofs, instances)"""
    setup = {"k8": w.s8, "k4": w.s4}[key]
    chosen = [pool[rnd.randrange(len(pool))] for _ in range(n)]
    if defect != "clean":
        at = rnd.randrange(n) if at is None else at
        chosen[at] = spoil(chosen[at][0], chosen[at][1], defect)
    return [(setup, p, i) for p, i in chosen], [p for p, _ in chosen], [i for _, i in chosen]


def draws_of(rnd, n, zero_at=None):
    d = [rnd.randrange(1, R_MOD) for _ in range(n)]
    if zero_at is not None:
        d[zero_at] = 0
    return d


# ------------------------------------------------------------------ pieces of schedules
def staged_round(w, rnd, pool, bname, route, sizes, defect, pairing=True, zero=False, reader=None, regroup=None):
    """one use of a staged batch: (configure,) upload by `route`, launch, finish, (a reader) -> [call]"""
    out = []
    if regroup == "sizes":
        out.append(call("b_set_group_sizes", bname, [bname], sizes=list(sizes)))
    elif regroup == "equal":
        out.append(call("b_set_groups", bname, [bname], groups=len(sizes)))
    n = sum(sizes)
    items, P, I = pick(w, rnd, pool, "k8", n, defect)
    draws = draws_of(rnd, n, zero_at=(1 + rnd.randrange(n - 1)) if zero and n > 1 else None)
    pf, inf = flat(P, I)
    up = dict(proofs=pf, proof_len=w.plen, instances=inf, col_lens=[8], rand=draw_bytes(draws))
    oks, st, lefts, rights, pair = launch_expect(w, items, draws, sizes, pairing)
    if route == "upload_launch":
        out.append(call("b_upload_launch", bname, [bname], pairing=pairing, **up))
    elif route == "tensors":
        out += [call("b_upload_tensors", bname, [bname], n=n, **up), call("b_launch", bname, [bname], pairing=pairing)]
        out.append(call("b_finish_into", bname, [bname], n=n, groups=len(sizes), expect={
            "status": st, "group_ok": [int(v) for v in oks], "left_xy": lefts, "right_xy": rights, "group_failed": rr.group_failed(st, sizes=list(sizes)),
            "summary": rr.summary(st, [int(v) for v in oks], len(sizes), rr.FLAG_PAIRING if pairing else 0)}))
    else:
        out += [call("b_upload", bname, [bname], **up), call("b_launch", bname, [bname], pairing=pairing)]
    out.append(call("b_finish_groups", bname, [bname], expect=(oks, st, lefts, rights)))
    off = offsets(sizes)
    if reader == "recheck":
        g = rnd.randrange(len(sizes))
        ranges = [(off[g], sizes[g]), (off[g] + rnd.randrange(sizes[g]), 1)]
        exp = [batch_reference.expected_range(items[off[g]:off[g + 1]], draws[off[g]:off[g + 1]], f - off[g], c) for f, c in ranges]
        out.append(call("b_recheck", bname, [bname], ranges=ranges, expect=([e[0] for e in exp], [e[1] for e in exp], [e[2] for e in exp])))
    elif reader == "identify":
        out.append(call("b_identify", bname, [bname], expect=([w.each(it) for it in items], pair)))
    return out


def batch_object(name, ctx, max_proofs=24, values=8, groups=1):
    return (name, "batch", ctx, {"max_proofs": max_proofs, "values": values, "groups": groups})


RAGGED = ([1, 5, 2, 4], [6, 1, 1], [3, 3, 3, 3, 3], [1, 23], [2, 7], [5])


def staged_thread(w, seed, t, bname, rounds, pool=None):
    """about `rounds` uses of one batch, alternating routes, readers and group layouts, with the thread's own proofs, draws and defects"""
    rnd = random.Random("staged/%s/%d" % (seed, t))
    pool = pool if pool is not None else w.own(t)
    out, sizes = [], [3, 3, 3, 3]
    out.append(call("b_set_groups", bname, [bname], groups=4))
    for r in range(rounds):
        kind = (r + t) % 5
        defect = DEFECTS[(r // 2 + t) % 4]
        if kind == 0:
            out += staged_round(w, rnd, pool, bname, "upload", sizes, defect, pairing=rnd.random() < 0.7, zero=rnd.random() < 0.5)
        elif kind == 1:
            out += staged_round(w, rnd, pool, bname, "upload_launch", sizes, defect, reader="recheck")
        elif kind == 2:
            out += staged_round(w, rnd, pool, bname, "tensors", sizes, defect, reader="identify")
        elif kind == 3:
            if (r // 5 + t) % 2 == 0:
                sizes = list(RAGGED[rnd.randrange(len(RAGGED))])
                out += staged_round(w, rnd, pool, bname, "upload", sizes, defect, reader="recheck", regroup="sizes")
            else:
                g = rnd.choice((1, 2, 4))
                sizes = [rnd.choice((1, 2, 6))] * g
                out += staged_round(w, rnd, pool, bname, "upload", sizes, defect, reader="recheck", regroup="equal")
        else:
            out += staged_round(w, rnd, pool, bname, "upload_launch", sizes, defect, reader="identify")
    return out


def verify_batch_call(w, rnd, pool, ctx, n, defect, os_draws=False, key="k8"):
    items, P, I = pick(w, rnd, pool, key, n, defect)
    if os_draws:     # statuses and the verdict only: a proof the pairing alone rejects fails the batch (but for 2^-254)
        st = [batch_reference.single(*it)[0] for it in items]
        ok = all(s == 0 and w.each(it) == 0 for s, it in zip(st, items))
        return call("verify_batch", ctx, proofs=P, instances=I, rand=None, expect=(ok, st, ANY, ANY))
    draws = draws_of(rnd, n)
    return call("verify_batch", ctx, proofs=P, instances=I, rand=draws, expect=w.expected(items, draws))


def verify_identify_call(w, rnd, pool, ctx, n, defect):
    items, P, I = pick(w, rnd, pool, "k8", n, defect)
    draws = draws_of(rnd, n)
    ok, _, left, right = w.expected(items, draws)
    return call("verify_batch_identify", ctx, proofs=P, instances=I, rand=draws, expect=(ok, [w.each(it) for it in items], left, right))


def verify_seeded_call(w, rnd, pool, ctx, n, defect):
    """the call that takes the context's lock four times: two MSMs over the seed, a pairing of it, the batch"""
    items, P, I = pick(w, rnd, pool, "k8", n, defect)
    draws = draws_of(rnd, n)
    sl, sr = w.points((w.s8,) + pool[rnd.randrange(len(pool))])
    a = rnd.randrange(1, R_MOD)
    seed = (([a, (1 - a) % R_MOD], [sl, sl]), ([1], [sr]))          # a L + (1 - a) L = L
    return call("verify_batch_seeded", ctx, proofs=P, instances=I, rand=draws, seed=seed, expect=w.expected(items, draws, seed=(sl, sr)))


def verify_batches_call(w, rnd, pool, ctx, sizes, defect):
    items, P, I = pick(w, rnd, pool, "k8", sum(sizes), defect)
    draws = draws_of(rnd, sum(sizes))
    off = offsets(sizes)
    batches = [(P[a:b], I[a:b]) for a, b in zip(off, off[1:])]
    return call("verify_batches", ctx, batches=batches, rand=draws, expect=[w.expected(items[a:b], draws[a:b]) for a, b in zip(off, off[1:])])


def verify_each_call(w, rnd, pool, ctx, n, defect):
    items, P, I = pick(w, rnd, pool, "k8", n, defect)
    return call("verify_each", ctx, proofs=P, instances=I, expect=[w.each(it) for it in items])


def guard_msm_call(w, rnd, pool, ctx):
    p, i = pool[rnd.randrange(len(pool))]
    rc, g = circuits.oracle_guard(w.s8, p, i)
    return call("guard_msm", ctx, proof=p, instances=i, expect=(rc, g))


def guards_call(w, rnd, pool, ctx, n, defect):
    items, _, _ = pick(w, rnd, pool, "k8", n, defect)
    return call("guards_check_each", ctx, guards=[w.guard(it) for it in items], expect=[w.pairing(*w.points(it)) for it in items])


def msm_g1_call(w, rnd, pool, ctx, n):
    bases = w.bases((w.s8,) + pool[rnd.randrange(len(pool))])
    sc = [rnd.randrange(R_MOD) for _ in range(n)]
    bs = [bases[rnd.randrange(len(bases))] for _ in range(n)]
    return call("msm_g1", ctx, scalars=sc, bases=bs, expect=w.msm(sc, bs))


def pairing_call(w, rnd, pool, ctx, good):
    left, right = w.points((w.s8,) + pool[rnd.randrange(len(pool))])
    if not good:
        right = w.points((w.s8,) + pool[(rnd.randrange(len(pool) - 1) + 1) % len(pool)])[0]
    return call("pairing_check", ctx, left=left, right=right, expect=w.pairing(left, right))


def msm_object_thread(w, seed, t, ctx, rounds, names):
    """an MSMKZG of the thread's own through append_terms / scale / scalars / eval_many, and dual_check_many over its DualMSM objects"""
    rnd = random.Random("msm/%s/%d" % (seed, t))
    pool = w.own(t)
    m1, m2, d1, d2 = names
    terms = {m1: ([], []), m2: ([], [])}
    bases = w.bases((w.s8,) + pool[0])
    out = []
    for r in range(rounds):
        m = (m1, m2)[r % 2]
        sc = [rnd.randrange(R_MOD) for _ in range(3)]
        bs = [bases[rnd.randrange(len(bases))] for _ in range(3)]
        out.append(call("msm_append", m, [m], scalars=sc, bases=bs))
        terms[m][0].extend(sc); terms[m][1].extend(bs)
        if r % 3 == 1:
            f = rnd.randrange(1, R_MOD)
            out.append(call("msm_scale", m, [m], factor=f))
            terms[m] = ([s * f % R_MOD for s in terms[m][0]], terms[m][1])
            out.append(call("msm_scalars", m, [m], expect=list(terms[m][0])))
        pts = [w.msm(*terms[m1]), w.msm(*terms[m2])]
        out.append(call("msm_eval_many", [m1, m2], [m1, m2], expect=(pts, [p == ZERO for p in pts])))
        out.append(call("dual_check_many", [d1, d2], [d1, d2], expect=dual_expect(w, [pool[1], spoil(*pool[2], "tamper")])))
    return out


def dual_object(w, name, ctx, proof):
    """a DualMSM holding one proof's Guard"""
    return (name, "dual", ctx, {"guard": w.guard((w.s8,) + tuple(proof))})


def dual_expect(w, proofs):
    pts = [w.points((w.s8,) + tuple(p)) for p in proofs]
    return [w.pairing(*p) for p in pts], [p[0] for p in pts], [p[1] for p in pts]


def accumulator_thread(w, seed, t, ctx, acc, rounds, every=1):
    """process, process_guards, add_msm and finalize on the thread's own accumulator"""
    rnd = random.Random("acc/%s/%d" % (seed, t))
    pool, model, out = w.own(t), AccModel(w), []
    for r in range(rounds):
        kind = r % 3
        if kind == 0:
            items, P, I = pick(w, rnd, pool, "k8", 3, DEFECTS[(r // 3 + t) % 4])
            draws = draws_of(rnd, 3)
            out.append(call("a_process", acc, [acc], contexts=ctx, keys=None, proofs=P, instances=I, rand=draws, expect=model.process(items, draws)))
        elif kind == 1:
            items, _, _ = pick(w, rnd, pool, "k8", 2, ("clean", "tamper")[(r // 3) % 2])
            draws = draws_of(rnd, 2)
            model.process(items, draws, guards=True)
            out.append(call("a_process_guards", acc, [acc], guards=[w.guard(it) for it in items], rand=draws))
        else:
            left, right = w.points((w.s8,) + pool[rnd.randrange(len(pool))])
            a = rnd.randrange(1, R_MOD)
            model.add(left, right)
            out.append(call("a_add_msm", acc, [acc], left=([a, (1 - a) % R_MOD], [left, left]), right=([1], [right])))
        if r % every == every - 1:
            out.append(call("a_finalize", acc, [acc], expect=model.finalize()))
    out.append(call("a_read", acc, [acc], expect=model.read()))
    return out


# ------------------------------------------------------------------ the scenes
def scene_first_use(w, seed, reps=5):
    """a fresh context per repetition, every thread released into the first calls the context ever sees"""
    out = []
    for rep in range(reps):     # (a) eight batches of one shape: one plan compile races seven cache hits, one split table is made once
        rnd = random.Random("first/a/%s/%d" % (seed, rep))
        threads = [staged_round(w, rnd, w.own(t), "b%d" % t, "upload", [6, 6, 6, 6], DEFECTS[(t + rep) % 4]) for t in range(8)]
        out.append({"contexts": [("ctx", "k8")], "objects": [batch_object("b%d" % t, "ctx", groups=4) for t in range(8)], "threads": threads, "main_after": [], "tag": "a"})
    for rep in range(reps):     # (b) eight different first calls
        rnd = random.Random("first/b/%s/%d" % (seed, rep))
        own = [w.own(t) for t in range(8)]
        model = AccModel(w)
        items, P, I = pick(w, rnd, own[3], "k8", 4, DEFECTS[rep % 4])
        draws = draws_of(rnd, 4)
        bases = w.bases((w.s8,) + own[7][0])
        sc = [rnd.randrange(R_MOD) for _ in range(5)]
        pt = w.msm(sc, bases[:5])
        threads = [
            [verify_batch_call(w, rnd, own[0], "ctx", 5, DEFECTS[(rep + 1) % 4])],
            [verify_each_call(w, rnd, own[1], "ctx", 4, DEFECTS[(rep + 2) % 4])],
            staged_round(w, rnd, own[2], "b", "upload", [3, 3], DEFECTS[(rep + 3) % 4]),
            [call("a_process", "acc", ["acc"], contexts="ctx", keys=None, proofs=P, instances=I, rand=draws, expect=model.process(items, draws)),
             call("a_finalize", "acc", ["acc"], expect=model.finalize())],
            [msm_g1_call(w, rnd, own[4], "ctx", 40)],
            [pairing_call(w, rnd, own[5], "ctx", rep % 2 == 0)],
            [guards_call(w, rnd, own[6], "ctx", 3, ("clean", "tamper")[rep % 2])],
            [call("msm_append", "m", ["m"], scalars=sc, bases=bases[:5]), call("msm_eval_many", ["m"], ["m"], expect=([pt], [pt == ZERO]))],
        ]
        out.append({"contexts": [("ctx", "k8")], "objects": [batch_object("b", "ctx", groups=2), ("acc", "acc", "ctx", {}), ("m", "msm", "ctx", {})],
                    "threads": threads, "main_after": [], "tag": "b"})
    return {"name": "first_use", "reps": out}


def scene_staged(w, seed, rounds=20):
    threads = [staged_thread(w, seed, t, "b%d" % t, rounds) for t in range(8)]
    return {"name": "staged", "reps": [{"contexts": [("ctx", "k8")], "objects": [batch_object("b%d" % t, "ctx") for t in range(8)], "threads": threads, "main_after": []}]}


def scene_plan_churn(w, seed):
    """40 instance shapes through a cache of 32 plans while other threads' batches hold pins"""
    threads = []
    for t in range(4):
        rnd = random.Random("churn/%s/%d" % (seed, t))
        order = list(range(1, 41))
        rnd.shuffle(order)
        calls = []
        for m in order:
            p, inst = w.shapes[m][t]
            d = draws_of(rnd, 1)
            calls += [call("b_upload", "b%d" % t, ["b%d" % t], proofs=p, proof_len=w.plen, instances=b"".join(inst[0]), col_lens=[m], rand=draw_bytes(d), shape=m),
                      call("b_launch", "b%d" % t, ["b%d" % t], pairing=True),
                      call("b_finish", "b%d" % t, ["b%d" % t], expect=w.expected([(w.s70, p, inst)], d))]
        threads.append(calls)
    for t in (4, 5):
        rnd = random.Random("churn/%s/%d" % (seed, t))
        calls = []
        for k in range(5):
            lens = rnd.sample(range(1, 41), 12)
            chosen = [w.shapes[m][t] for m in lens]
            if k % 2:
                at = rnd.randrange(12)
                chosen[at] = spoil(chosen[at][0], chosen[at][1], "input")
            items = [(w.s70, p, i) for p, i in chosen]
            d = draws_of(rnd, 12)
            calls.append(call("verify_batch_shapes", "ctx", proofs=[p for p, _ in chosen], instances=[i for _, i in chosen], rand=d, shapes=lens,
                              expect=w.expected(items, d)))
        threads.append(calls)
    return {"name": "plan_churn", "reps": [{"contexts": [("ctx", "k70")], "objects": [batch_object("b%d" % t, "ctx", 1, 70) for t in range(4)],
                                            "threads": threads, "main_after": []}]}


def churn_shapes_under_pins(scene):
    """from the schedule: the fewest distinct shapes a thread uploads while another thread's batch holds a plan (every batch holds the
    plan of its last upload until the next one, so from its first upload on every other walker holds one)"""
    rep = scene["reps"][0]
    walkers = [[c["args"]["shape"] for c in th if c["op"] == "b_upload"] for th in rep["threads"]]
    walkers = [s for s in walkers if s]
    assert len(walkers) >= 2
    return min(len(set(s)) for s in walkers)


def scene_oneshot_mix(w, seed, rounds=16):
    """one thread per one-shot entry point (some threads two), beside two staged batches and an accumulator"""
    R = lambda t: random.Random("mix/%s/%d" % (seed, t))
    own = [w.own(t) for t in range(8)]
    threads = [[] for _ in range(8)]
    r0, r1, r2, r3 = R(0), R(1), R(2), R(3)
    for r in range(rounds):
        d = DEFECTS[r % 4]
        threads[0] += [verify_batch_call(w, r0, own[0], "ctx", 3 + r % 4, d, os_draws=r % 5 == 4), verify_identify_call(w, r0, own[0], "ctx", 6, DEFECTS[(r + 1) % 4]),
                       msm_g1_call(w, r0, own[0], "ctx", 30 + r)]
        threads[1] += [verify_seeded_call(w, r1, own[1], "ctx", 4, DEFECTS[(r + 2) % 4]), verify_batches_call(w, r1, own[1], "ctx", [2, 3, 1], DEFECTS[(r + 3) % 4])]
        threads[2] += [verify_each_call(w, r2, own[2], "ctx", 4, d), guard_msm_call(w, r2, own[2], "ctx"), msm_g1_call(w, r2, own[2], "ctx", 20 + r)]
        threads[3] += [guards_call(w, r3, own[3], "ctx", 3, ("clean", "tamper", "input")[r % 3]), msm_g1_call(w, r3, own[3], "ctx", 5 + 7 * r),
                       pairing_call(w, r3, own[3], "ctx", r % 2 == 0)]
        # h2v_msm_g1 from four threads in every round, short calls back to back: a result that leaves through state another caller
        # already owns has the most chances here
        for t, rt in enumerate((r0, r1, r2, r3)):
            threads[t] += [msm_g1_call(w, rt, own[t], "ctx", 1 + (r + k + t) % 4) for k in range(3)]
    threads[4] = msm_object_thread(w, seed, 4, "ctx", rounds, ("m1", "m2", "d1", "d2"))
    threads[5] = staged_thread(w, seed + 50, 5, "b5", rounds)
    threads[6] = staged_thread(w, seed + 50, 6, "b6", rounds)
    threads[7] = accumulator_thread(w, seed, 7, "ctx", "acc", 2 * rounds)
    objects = [("m1", "msm", "ctx", {}), ("m2", "msm", "ctx", {}), dual_object(w, "d1", "ctx", own[4][1]), dual_object(w, "d2", "ctx", spoil(*own[4][2], "tamper")),
               batch_object("b5", "ctx"), batch_object("b6", "ctx"), ("acc", "acc", "ctx", {})]
    return {"name": "oneshot_mix", "reps": [{"contexts": [("ctx", "k8")], "objects": objects, "threads": threads, "main_after": []}]}


def scene_two_contexts(w, seed, rounds=30):
    """contexts A and B over the same params; pairs of threads make the same call with the contexts the other way round, round by round"""
    setups = {"A": w.s8, "B": w.s4}
    pools = {"A": w.pool8, "B": w.pool4}
    threads = [[] for _ in range(8)]
    objects = []
    rnds = [random.Random("two/%s/%d" % (seed, t)) for t in range(8)]

    def mixed(rnd, t, order, n, defect):
        """n proofs alternating between the two keys, from the thread's own part of each pool"""
        items, P, I, keys = [], [], [], []
        for j in range(n):
            k = j % 2
            name = order[k]
            share = pools[name][t * 3:(t + 1) * 3]
            p, i = share[rnd.randrange(3)]
            if defect != "clean" and j == 1:
                p, i = spoil(p, i, defect)
            items.append((setups[name], p, i)); P.append(p); I.append(i); keys.append(k)
        return items, P, I, keys

    # the objects of the MSM pairs: a destination on one context, a source on the other, for threads 2 and 3
    msm_terms = {}
    msm_order = {2: ["A", "B"], 3: ["B", "A"]}
    for t, (dst, src) in ((2, ("A", "B")), (3, ("B", "A"))):
        bases = w.bases((w.s8,) + w.own(t)[0])
        assert len(bases) >= 3 * t + 3
        sc = [rnds[t].randrange(R_MOD) for _ in range(3)]
        msm_terms[t] = [[], []], (sc, bases[3 * t:3 * t + 3])
        objects += [("dst%d" % t, "msm", dst, {}), ("src%d" % t, "msm", src, {"terms": msm_terms[t][1]})]
    for t, order in ((4, ("A", "B")), (5, ("B", "A"))):
        objects += [dual_object(w, "dual%d%s" % (t, c), c, w.own(t)[k] if k == 0 else spoil(*w.own(t)[k], "tamper")) for k, c in enumerate(order)]
    objects += [("acc6", "acc", "A", {}), ("acc7", "acc", "B", {})]
    models = {6: AccModel(w), 7: AccModel(w)}
    for r in range(rounds):
        d = DEFECTS[r % 4]
        for t, order in ((0, ("A", "B")), (1, ("B", "A"))):
            items, P, I, keys = mixed(rnds[t], t, order, 4, d)
            draws = draws_of(rnds[t], 4)
            threads[t].append(call("verify_batch_keys", list(order), round=r, order=list(order), keys=keys, proofs=P, instances=I, rand=draws,
                                   expect=w.expected(items, draws)))
        for t in (2, 3):
            acc, src = msm_terms[t]
            acc[0].extend(src[0]); acc[1].extend(src[1])
            threads[t].append(call("msm_add_msm", ["dst%d" % t, "src%d" % t], ["dst%d" % t, "src%d" % t], round=r, order=msm_order[t]))
            if r % 5 == 4:
                pt = w.msm(*acc)
                threads[t].append(call("msm_eval_many", ["dst%d" % t], ["dst%d" % t], expect=([pt], [pt == ZERO])))
        for t, order in ((4, ("A", "B")), (5, ("B", "A"))):
            names = ["dual%d%s" % (t, c) for c in order]
            threads[t].append(call("dual_check_many", names, names, round=r, order=list(order), expect=dual_expect(w, [w.own(t)[0], spoil(*w.own(t)[1], "tamper")])))
        for t, order in ((6, ("A", "B")), (7, ("B", "A"))):
            items, P, I, keys = mixed(rnds[t], t, order, 4, DEFECTS[(r + 2) % 4])
            draws = draws_of(rnds[t], 4)
            threads[t].append(call("a_process", "acc%d" % t, ["acc%d" % t], round=r, order=list(order), contexts=list(order), keys=keys, proofs=P, instances=I, rand=draws,
                                   expect=models[t].process(items, draws)))
            if r % 10 == 9:
                threads[t].append(call("a_finalize", "acc%d" % t, ["acc%d" % t], expect=models[t].finalize()))
    return {"name": "two_contexts", "reps": [{"contexts": [("A", "k8"), ("B", "k4")], "objects": objects, "threads": threads, "main_after": [], "barrier_rounds": True}]}


def scene_feeders(w, seed, rounds=4):
    """four feeder threads, an accumulator each; the main thread merges them"""
    threads, models, objects = [], [], []
    for t in range(4):
        rnd = random.Random("feed/%s/%d" % (seed, t))
        pool, model, acc, b = w.own(t), AccModel(w), "acc%d" % t, "b%d" % t
        objects += [(acc, "acc", "ctx", {}), batch_object(b, "ctx")]
        calls = [call("b_set_groups", b, [b], groups=2)]
        for r in range(rounds):
            defect = {(1, 0): "tamper", (2, 1): "noncanon"}.get((t, r), "clean")     # feeder 1's own pairing fails; feeder 2 counts a failed proof
            items, P, I = pick(w, rnd, pool, "k8", 3, defect)
            draws = draws_of(rnd, 3)
            calls.append(call("a_process", acc, [acc], contexts="ctx", keys=None, proofs=P, instances=I, rand=draws, expect=model.process(items, draws)))
            items, _, _ = pick(w, rnd, pool, "k8", 2, "clean")
            draws = draws_of(rnd, 2)
            model.process(items, draws, guards=True)
            calls.append(call("a_process_guards", acc, [acc], guards=[w.guard(it) for it in items], rand=draws))
            # a staged batch of its own, two groups of two, fed as two legs
            items, P, I = pick(w, rnd, pool, "k8", 4, "clean")
            draws = draws_of(rnd, 4)
            pf, inf = flat(P, I)
            oks, st, lefts, rights, _ = launch_expect(w, items, draws, [2, 2])
            calls += [call("b_upload_launch", b, [b], pairing=True, proofs=pf, proof_len=w.plen, instances=inf, col_lens=[8], rand=draw_bytes(draws)),
                      call("b_finish_groups", b, [b], expect=(oks, st, lefts, rights))]
            model.process(items[:2], draws[:2]); model.process(items[2:], draws[2:])
            calls.append(call("a_process_batch", acc, [acc, b], batch=b, expect=(4, 0)))
        state = model.read()
        calls.append(call("a_read", acc, [acc], expect=state))
        calls.append(call("a_export_state", acc, [acc], expect=rr_pack_state(*state)))
        threads.append(calls)
        models.append(model)
    rnd = random.Random("feed/%s/main" % seed)
    c = draws_of(rnd, 4)
    states = [m.read() for m in models]
    left, right = w.msm(c, [s[0] for s in states]), w.msm(c, [s[1] for s in states])
    n, failed = sum(s[2] for s in states), sum(s[3] for s in states)
    ok = not failed and w.pairing(left, right)
    bits = [int(w.pairing(s[0], s[1])) for s in states]
    names = ["acc%d" % t for t in range(4)]
    objects.append(("dst", "acc", "ctx", {}))
    main_after = [call("a_merge", "dst", ["dst"] + names, sources=names, draws=c, expect=[le32(x) for x in c]),
                  call("a_read", "dst", ["dst"], expect=(left, right, n, failed)),
                  call("a_finalize", "dst", ["dst"], expect=(ok, left, right)),
                  call("merge_local", "ctx", names, sources=names, draws=c, expect=(ok, left, right, bits))]
    return {"name": "feeders", "reps": [{"contexts": [("ctx", "k8")], "objects": objects, "threads": threads, "main_after": main_after}]}


def rr_pack_state(left, right, n, failed):
    """include/h2v.h: [u32 magic "H2VS"][u32 version 1][u64 n_proofs][u64 n_failed][left x | y][right x | y], little-endian"""
    import struct
    return struct.pack("<IIQQ", 0x53563248, 1, n, failed) + left + right


def scene_errors(w, seed, rounds=4):
    """every thread provokes refusals of its own, with its own text, between successful calls: argument refusals only"""
    threads, objects = [], []
    off_curve = le32(1) + le32(1)         # (1, 1): y^2 != x^3 + 3
    for t in range(8):
        rnd = random.Random("err/%s/%d" % (seed, t))
        pool = w.own(t)
        bases = w.bases((w.s8,) + pool[0])
        good = [w.guard((w.s8,) + pool[k % len(pool)]) for k in range(t + 2)]
        side = t % 2
        bad = [list(map(list, g)) for g in good]
        bad[t][side] = [list(bad[t][side][0]), [off_curve] + list(bad[t][side][1][1:])]
        guard_text = "h2v_guards_check_each: guard %d, %s side: a scalar that is not canonical, or a base that is neither all-zero nor a canonical point on the curve" % (
            t, ("left", "right")[side])
        shapes65 = [[[le32(1)] * m] for m in range(65)]
        refusals = [
            lambda: call("msm_g1", "ctx", scalars=[3, R_MOD + t], bases=bases[:2], error=(BAD_ARGUMENT, "h2v_msm_g1: scalar not canonical")) if t % 2 == 0 else
            call("msm_g1", "ctx", scalars=[3, 4], bases=[bases[0], off_curve], error=(BAD_ARGUMENT, "h2v_msm_g1: base not on the curve")),
            lambda: call("pairing_check", "ctx", left=off_curve, right=bases[0], error=(BAD_ARGUMENT, "h2v_pairing_check: point not on the curve")),
            lambda: call("b_launch", "b%d" % t, ["b%d" % t], pairing=True, error=(BAD_ARGUMENT, "h2v_batch_launch: nothing uploaded since the last failed call or set_groups")),
            lambda: call("verify_batch_shapes", "ctx70", proofs=[w.shapes[1][0][0]] * 65, instances=shapes65, rand=[1] * 65, shapes=list(range(65)),
                         error=(UNSUPPORTED, "more than 64 distinct (key, instance shape) groups in one call")),
            lambda: call("guards_check_each", "ctx", guards=bad, error=(BAD_ARGUMENT, guard_text)),
        ]
        calls = []
        for r in range(rounds):
            for k in range(5):
                calls.append(refusals[(k + t) % 5]())
                calls.append(msm_g1_call(w, rnd, pool, "ctx", 8 + t) if (k + r) % 2 else pairing_call(w, rnd, pool, "ctx", (r + t) % 2 == 0))
        threads.append(calls)
        objects.append(batch_object("b%d" % t, "ctx"))
    return {"name": "errors", "reps": [{"contexts": [("ctx", "k8"), ("ctx70", "k70")], "objects": objects, "threads": threads, "main_after": []}]}


def scene_hand_over(w, seed, rounds=10):
    """objects move between threads without ever being used by two at once: a batch uploaded on thread 0, launched on 1 and finished on
    2, round after round; an accumulator created on the main thread, fed on thread 3 and finalised on the main thread"""
    rnd = random.Random("hand/%s" % seed)
    threads = [[], [], [], []]
    for r in range(rounds):
        one = staged_round(w, rnd, w.own(r % 8), "b", "upload", [3, 3], DEFECTS[r % 4])
        up, launch, finish = one
        up["after"] = (2, r - 1) if r else None
        launch["after"] = (0, r)
        finish["after"] = (1, r)
        threads[0].append(up); threads[1].append(launch); threads[2].append(finish)
    model = AccModel(w)
    for r in range(3):
        items, P, I = pick(w, rnd, w.own(3), "k8", 3, DEFECTS[r])
        draws = draws_of(rnd, 3)
        threads[3].append(call("a_process", "acc", ["acc"], contexts="ctx", keys=None, proofs=P, instances=I, rand=draws, expect=model.process(items, draws)))
    main_after = [call("a_finalize", "acc", ["acc"], expect=model.finalize()), call("a_read", "acc", ["acc"], expect=model.read())]
    objects = [batch_object("b", "ctx", groups=2), ("acc", "acc", "ctx", {})]
    return {"name": "hand_over", "reps": [{"contexts": [("ctx", "k8")], "objects": objects, "threads": threads, "main_after": main_after}]}


ACC_RECORD_BYTES = 1312        # include/h2v.h H2V_ACC_RECORD_BYTES
ACC_POINTS_BYTES = 216         # h2v_batch_accumulators: per group [left, right], 2 x 108 bytes


def scene_same_call(w, seed):
    """every entry point from eight threads at the same moment: the threads walk one menu of calls in step, a barrier in front of every
    call, each with inputs and objects of its own — so that no entry point is only ever called by one thread at a time"""
    threads, objects = [], []
    for t in range(8):
        rnd = random.Random("same/%s/%d" % (seed, t))
        pool, pool4 = w.own(t), w.pool4[t * 3:(t + 1) * 3]
        b, acc, accj, accd, m, n2, d, e = ["%s%d" % (x, t) for x in ("b", "acc", "accj", "accd", "m", "n", "d", "e")]
        objects += [batch_object(b, "A"), (acc, "acc", "A", {}), (accj, "acc", "A", {}), (accd, "acc", "A", {}), (m, "msm", "A", {}), (n2, "msm", "A", {}),
                    dual_object(w, d, "A", pool[1]), dual_object(w, e, "A", spoil(*pool[2], "tamper"))]
        out, model = [], AccModel(w)
        D = lambda k: DEFECTS[(t + k) % 4]
        # the one-shot entry points
        out += [verify_batch_call(w, rnd, pool, "A", 4, D(0)), verify_seeded_call(w, rnd, pool, "A", 3, D(1))]
        chosen = [w.shapes[1 + t + 8 * j][t % 6] for j in range(3)]
        draws = draws_of(rnd, 3)
        out.append(call("verify_batch_shapes", "C", proofs=[p for p, _ in chosen], instances=[i for _, i in chosen], rand=draws,
                        expect=w.expected([(w.s70, p, i) for p, i in chosen], draws)))
        out.append(verify_identify_call(w, rnd, pool, "A", 5, D(2)))
        items, P, I = pick(w, rnd, pool, "k8", 4, D(3))
        draws = draws_of(rnd, 4)
        sl, sr = w.points((w.s8,) + pool[3])
        ok, _, left, right = w.expected(items, draws, seed=(sl, sr))
        out.append(call("verify_batch_seeded_identify", "A", proofs=P, instances=I, rand=draws, seed=(([1], [sl]), ([1], [sr])),
                        expect=(ok, [w.each(it) for it in items], left, right)))
        out += [verify_batches_call(w, rnd, pool, "A", [1, 3, 2], D(0)), verify_each_call(w, rnd, pool, "A", 4, D(1))]
        for identify in (False, True):
            chosen = [pool[0], pool4[0], spoil(*pool[1], D(2)) if identify else pool[1], pool4[1]]
            items = [((w.s8, w.s4)[j % 2],) + tuple(c) for j, c in enumerate(chosen)]
            draws = draws_of(rnd, 4)
            ok, st, left, right = w.expected(items, draws)
            args = dict(keys=[0, 1, 0, 1], proofs=[c[0] for c in chosen], instances=[c[1] for c in chosen], rand=draws)
            if identify:
                out.append(call("verify_batch_keys_identify", ["A", "B"], expect=(ok, [w.each(it) for it in items], left, right), **args))
            else:
                out.append(call("verify_batch_keys", ["A", "B"], expect=(ok, st, left, right), **args))
        out += [guard_msm_call(w, rnd, pool, "A"), guards_call(w, rnd, pool, "A", 3, ("clean", "tamper")[t % 2]), msm_g1_call(w, rnd, pool, "A", 20 + t),
                pairing_call(w, rnd, pool, "A", t % 2 == 0)]
        # the MSM objects
        bases = w.bases((w.s8,) + pool[0])
        tm = ([rnd.randrange(R_MOD) for _ in range(4)], [bases[rnd.randrange(len(bases))] for _ in range(4)])
        tn = ([rnd.randrange(R_MOD) for _ in range(3)], [bases[rnd.randrange(len(bases))] for _ in range(3)])
        f = rnd.randrange(1, R_MOD)
        scaled = [x * f % R_MOD for x in tm[0]]
        whole = (scaled + tn[0], tm[1] + tn[1])
        pts = [w.msm(*whole), w.msm(*tn)]
        out += [call("msm_append", m, [m], scalars=tm[0], bases=tm[1]), call("msm_append", n2, [n2], scalars=tn[0], bases=tn[1]),
                call("msm_scale", m, [m], factor=f), call("msm_scalars", m, [m], expect=scaled), call("msm_add_msm", [m, n2], [m, n2]),
                call("msm_eval_many", [m, n2], [m, n2], expect=(pts, [p == ZERO for p in pts])),
                call("dual_check_many", [d, e], [d, e], expect=dual_expect(w, [pool[1], spoil(*pool[2], "tamper")])),
                call("a_add_msms", acc, [acc, d], dual=d)]
        model.add(*w.points((w.s8,) + pool[1]))
        # the staged batch: equal groups, unequal groups, from device memory
        out.append(call("b_set_groups", b, [b], groups=4))
        first = staged_round(w, rnd, pool, b, "upload", [3, 3, 3, 3], D(3), reader="recheck")
        ranges = first[-1]["args"]["ranges"]
        out += first
        out.append(call("b_recheck_many", b, [b], ranges=[(0, fr, c) for fr, c in ranges]))
        out[-1]["expect"] = first[-1]["expect"]
        out += staged_round(w, rnd, pool, b, "upload_launch", [1, 5, 2, 4], D(0), reader="identify", regroup="sizes")
        sizes = [2, 7]
        n = sum(sizes)
        items, P, I = pick(w, rnd, pool, "k8", n, D(1))
        draws = draws_of(rnd, n)
        pf, inf = flat(P, I)
        oks, st, lefts, rights, _ = launch_expect(w, items, draws, sizes)
        out += [call("b_set_group_sizes", b, [b], sizes=sizes),
                call("b_upload_tensors", b, [b], n=n, proofs=pf, proof_len=w.plen, instances=inf, col_lens=[8], rand=draw_bytes(draws)),
                call("b_launch", b, [b], pairing=True),
                call("b_finish_into", b, [b], n=n, groups=2, expect={
                    "status": st, "group_ok": [int(v) for v in oks], "left_xy": lefts, "right_xy": rights, "group_failed": rr.group_failed(st, sizes=sizes),
                    "summary": rr.summary(st, [int(v) for v in oks], 2, rr.FLAG_PAIRING)}),
                call("b_finish_groups", b, [b], expect=(oks, st, lefts, rights))]
        off = offsets(sizes)
        for a0, a1 in zip(off, off[1:]):
            model.process(items[a0:a1], draws[a0:a1])
        out.append(call("a_process_batch", acc, [acc, b], batch=b, expect=(n, sum(1 for v in st if v))))
        # one group, closed by a fold of its own exported record (a sharded run of one rank), and by h2v_fold_check
        items, P, I = pick(w, rnd, pool, "k8", 5, ("clean", "tamper")[t % 2])
        draws = draws_of(rnd, 5)
        pf, inf = flat(P, I)
        oks, st, lefts, rights, _ = launch_expect(w, items, draws, [5])
        rec = "rec%d" % t
        out += [call("b_set_groups", b, [b], groups=1), call("b_upload", b, [b], proofs=pf, proof_len=w.plen, instances=inf, col_lens=[8], rand=draw_bytes(draws)),
                call("b_launch", b, [b], pairing=False), call("b_accumulators", b, [b], expect=ACC_POINTS_BYTES),
                call("b_export", b, [b, rec], rec=rec, groups=1), call("fold_check", "A", [rec], rec=rec, expect=(oks[0], lefts[0], rights[0])),
                call("b_fold_enqueue", b, [b, rec], rec=rec), call("b_finish", b, [b], expect=(oks[0], st, lefts[0], rights[0]))]
        # on a stream of the caller's
        items, P, I = pick(w, rnd, pool, "k8", 4, D(2))
        draws = draws_of(rnd, 4)
        pf, inf = flat(P, I)
        oks, st, lefts, rights, _ = launch_expect(w, items, draws, [4])
        out += [call("b_set_stream", b, [b], stream="stream%d" % t), call("b_upload", b, [b], proofs=pf, proof_len=w.plen, instances=inf, col_lens=[8], rand=draw_bytes(draws)),
                call("b_launch", b, [b], pairing=True), call("b_finish", b, [b], expect=(oks[0], st, lefts[0], rights[0]))]
        # the accumulators: feeding, the journal, merging
        items, P, I = pick(w, rnd, pool, "k8", 3, "clean")
        draws = draws_of(rnd, 3)
        out.append(call("a_process", acc, [acc], contexts="A", keys=None, proofs=P, instances=I, rand=draws, expect=model.process(items, draws)))
        items, _, _ = pick(w, rnd, pool, "k8", 2, "clean")
        draws = draws_of(rnd, 2)
        model.process(items, draws, guards=True)
        out.append(call("a_process_guards", acc, [acc], guards=[w.guard(it) for it in items], rand=draws))
        left, right = w.points((w.s8,) + pool[4])
        model.add(left, right)
        out += [call("a_add_msm", acc, [acc], left=([1], [left]), right=([1], [right])), call("a_read", acc, [acc], expect=model.read()),
                call("a_finalize", acc, [acc], expect=model.finalize()), call("a_export_state", acc, [acc], expect=rr_pack_state(*model.read()))]
        kept = AccModel(w)
        leg1, P1, I1 = pick(w, rnd, pool, "k8", 3, "clean")
        leg2, P2, I2 = pick(w, rnd, pool, "k8", 3, "tamper")
        d1, d2 = draws_of(rnd, 3), draws_of(rnd, 3)
        alone = AccModel(w)
        alone.process(leg2, d2)
        out += [call("a_journal_begin", accj, [accj], capacity=8),
                call("a_process", accj, [accj], contexts="A", keys=None, proofs=P1, instances=I1, rand=d1, expect=kept.process(leg1, d1)),
                call("a_process", accj, [accj], contexts="A", keys=None, proofs=P2, instances=I2, rand=d2, expect=[0, 0, 0]),
                call("a_check_legs", accj, [accj], expect=[(0, 0, True), (3, 0, kept.finalize()[0]), (3, 0, alone.finalize()[0])]),
                call("a_drop_legs", accj, [accj], legs=[2]), call("a_read", accj, [accj], expect=kept.read())]
        c1, c2 = draws_of(rnd, 2)
        sa, sj = model.read(), kept.read()
        merged = (w.msm([c1, c2], [sa[0], sj[0]]), w.msm([c1, c2], [sa[1], sj[1]]), sa[2] + sj[2], sa[3] + sj[3])
        out += [call("a_merge", accd, [accd, acc], sources=[acc], draws=[c1], expect=[le32(c1)]),
                call("a_merge_states", accd, [accd], states=[rr_pack_state(*sj)], draws=[c2], expect=[le32(c2)]),
                call("a_read", accd, [accd], expect=merged)]
        # the two shortest calls on a batch return within nanoseconds: two more rounds each, 32 calls in a row per thread and round
        for k in range(2):
            out += [call("b_stream", b, [b], repeat=32, expect=True), call("b_set_groups", b, [b], groups=(1, 2, 4)[k % 3], repeat=32)]
        out.append(call("msm_g1", "A", scalars=[R_MOD + t + 1], bases=bases[:1], error=(BAD_ARGUMENT, "h2v_msm_g1: scalar not canonical")))
        for k, c in enumerate(out):
            c["round"] = k
        threads.append(out)
    assert len({tuple(c["op"] for c in th) for th in threads}) == 1      # in step: the same call in every round
    return {"name": "same_call", "reps": [{"contexts": [("A", "k8"), ("B", "k4"), ("C", "k70")], "objects": objects, "threads": threads, "main_after": [],
                                           "barrier_rounds": True}]}


SCENES = ("first_use", "staged", "plan_churn", "oneshot_mix", "two_contexts", "feeders", "errors", "hand_over", "same_call")
SEED = 20240


def build(seed=SEED, world=None):
    """-> {"keys", "scenes"}: everything tests/thread_driver.py needs, as plain data"""
    w = world or World(seed)
    try:
        scenes = [scene_first_use(w, seed), scene_staged(w, seed), scene_plan_churn(w, seed), scene_oneshot_mix(w, seed), scene_two_contexts(w, seed),
                  scene_feeders(w, seed), scene_errors(w, seed), scene_hand_over(w, seed), scene_same_call(w, seed)]
    finally:
        if world is None:
            w.free()
    assert tuple(s["name"] for s in scenes) == SCENES
    return {"keys": w.keys, "scenes": scenes}


# ------------------------------------------------------------------ what the schedules promise (tests/test_thread_scenes_host.py)
def all_calls(rep):
    """[(thread, index, call)], the main thread's calls behind the others as thread -1"""
    out = [(t, i, c) for t, th in enumerate(rep["threads"]) for i, c in enumerate(th)]
    return out + [(-1, i, c) for i, c in enumerate(rep["main_after"])]


def shared_object_conflicts(rep):
    """pairs of calls that use one object from two threads with no order between them: program order in a thread, `after` edges, and
    the main thread's calls behind every thread's last.  [] is the contract."""
    calls = all_calls(rep)
    index = {(t, i): k for k, (t, i, _) in enumerate(calls)}
    n = len(calls)
    before = [set() for _ in range(n)]         # direct predecessors
    for k, (t, i, c) in enumerate(calls):
        if i > 0:
            before[k].add(index[(t, i - 1)])
        if c["after"] is not None:
            before[k].add(index[tuple(c["after"])])
        if t == -1 and i == 0:
            before[k].update(index[(u, len(th) - 1)] for u, th in enumerate(rep["threads"]) if th)
    users = {}
    for k, (t, i, c) in enumerate(calls):
        for name in c["uses"]:
            users.setdefault(name, []).append(k)
    reach = {}

    def ancestors(k):
        if k not in reach:
            seen, todo = set(), list(before[k])
            while todo:
                j = todo.pop()
                if j not in seen:
                    seen.add(j)
                    todo.extend(before[j])
            reach[k] = seen
        return reach[k]

    bad = []
    for name, ks in users.items():
        if len({calls[k][0] for k in ks}) < 2:
            continue                            # one thread's own object
        for a in ks:
            for b in ks:
                if a < b and calls[a][0] != calls[b][0] and a not in ancestors(b) and b not in ancestors(a):
                    bad.append((name, calls[a][:2], calls[b][:2]))
    return bad


def symbols_reached(scene):
    """C symbol -> the number of threads of one repetition whose schedule calls it (the most over the repetitions)"""
    out = {}
    for rep in scene["reps"]:
        per = {}
        for t, _, c in all_calls(rep):
            for sym in OP_SYMBOLS[c["op"]] + (ERROR_SYMBOLS if c["error"] else ()):
                per.setdefault(sym, set()).add(t)
        for sym, ts in per.items():
            out[sym] = max(out.get(sym, 0), len(ts))
    return out
