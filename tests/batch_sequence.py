"""Model-based sequences of calls on ONE long-lived Batch and its Context (host only: nothing here touches the GPU library).

A staged batch carries state from one use to the next — the stage, the pinned plan, grow-only buffers, `decompressed`,
`mult_of_draws`, `device_draws`, `zero_below`, the group offsets on the device, scratch words that are zero "between calls", the
context's scratch batch and plan cache.  Each of those invariants was tested with its own two-step sequence; this module generates
long ones:

  * an operation alphabet (Step): configure, upload by four routes, launch, seven readers, one-shot context calls, a second batch in
    flight, and calls the current stage refuses;
  * a model (Model) that says for every step "refused with code c, state unchanged", "refused, batch now Empty" or "values", and
    keeps what the values depend on (View);
  * the values themselves (Expect), only from the references the suite already has: batch_reference (linearity over the oracle's
    per-proof Guards), results_reference, record_reference, oracle_lib.g1_msm and circuits.oracle_*;
  * a seeded generator (sequence) with a `focus`, and a trace printer (trace) whose lines are Python: `run.upload(route='device', ...)`
    replays the step on the driver object of tests/test_gpu_batch_sequence.py.

CASES is the committed list of (seed, focus, steps); tests/test_batch_sequence_host.py holds it to the coverage conditions."""
import collections
import random

import batch_reference
from circuits import R_MOD

EMPTY, UPLOADED, LAUNCHED, FINISHED = 0, 1, 2, 3
STAGE_NAMES = ("Empty", "Uploaded", "Launched", "Finished")
BAD_ARGUMENT = -16

CAPACITY = 320
ROUTES = ("upload", "upload_launch", "device", "device_os")
HOST_ROUTES = ("upload", "upload_launch")
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 300)     # either side of a wave and of MULT_TILE / RESULTS_TILE (256)
SHAPES = (8, 5, 3, 0)                               # public inputs of a proof: one plan each
GROUPS = (1, 2, 4, 8)
# unequal groups: 2 - 5 of them, a group of one proof, a group that holds proofs 63 and 64
RAGGED = ([1, 62, 2], [1, 100, 155], [1, 62, 2, 190, 2], [255, 1, 44], [1, 60, 194], [1, 59, 5])
DRAWS = ("random", "ones", "alternating", "zero_at")
CONTENT = ("clean", "input", "point", "eval", "sign", "two")
READERS = ("finish", "finish_groups", "finish_into", "recheck", "identify", "export", "process_batch")
OUTPUTS = ("status", "group_ok", "left_xy", "right_xy", "group_failed", "failed_index", "summary")
CTX_KINDS = ("verify_batch", "verify_each", "verify_batch_identify", "guard_msm", "msm_g1", "eval_many")
FOCUSES = ("sizes", "groups", "routes", "readers", "context")

# the least stage every call accepts (csrc/batch.hip require_stage, accumulator.hip for process_batch)
LEAST = {"launch": UPLOADED, "finish": LAUNCHED, "finish_groups": LAUNCHED, "finish_into": LAUNCHED, "export": LAUNCHED,
         "recheck": FINISHED, "identify": FINISHED, "process_batch": FINISHED}
# refusals that depend on more than the stage: (call, the stages it is generated at)
CONDITIONAL = {"finish_grouped": (LAUNCHED, FINISHED),      # h2v_batch_finish on a grouped batch
               "export_ragged": (LAUNCHED, FINISHED),       # records count the failures of n / groups proofs
               "recheck_cross": (FINISHED,),                # a range over two groups
               "recheck_zero": (FINISHED,),                 # a range over a proof whose multiplier is zero
               "identify_zero": (FINISHED,)}


def illegal_table():
    """every (stage, call) the model refuses with BAD_ARGUMENT and no change of state"""
    rows = [(st, call) for call, least in LEAST.items() for st in range(least)]
    rows += [(st, call) for call, stages in CONDITIONAL.items() for st in stages]
    return sorted(rows)


class Step:
    """one call: `op` is a method of the driver, `kw` its keyword arguments (plain data)"""
    __slots__ = ("op", "kw")

    def __init__(self, op, **kw):
        self.op, self.kw = op, kw

    def line(self):
        return "run.%s(%s)" % (self.op, ", ".join("%s=%r" % kv for kv in self.kw.items()))

    __repr__ = line


def trace(steps):
    """one line of Python per step"""
    return "\n".join(s.line() for s in steps)


View = collections.namedtuple("View", "up groups sizes pairing fault")
Outcome = collections.namedtuple("Outcome", "kind code view")   # kind: "ok" | "refused" (state unchanged) | "refused_empty"


# ------------------------------------------------------------------ what an upload holds (pure functions of its keywords)
def group_sizes(n, groups, sizes):
    return list(sizes) if sizes is not None else [n // groups] * groups


def group_offsets(n, groups, sizes):
    off = [0]
    for s in group_sizes(n, groups, sizes):
        off.append(off[-1] + s)
    assert off[-1] == n, (n, groups, sizes)
    return off


def zero_pos(up):
    return 1 + (up["seed"] * 31) % (up["n"] - 1)


def draws_of(up):
    """the draws as uploaded (a bad draw included), or None for OS draws"""
    if up["route"] == "device_os":
        return None
    n, kind = up["n"], up["draws"]
    d = batch_reference.pattern_draws(kind, n, seed=1000 + up["seed"], k=zero_pos(up) if kind == "zero_at" else None)
    bad = up.get("bad_draw")
    if bad is not None:
        d[bad] = R_MOD + up["seed"] % 5
        if bad < n - 1:
            d[n - 1] = R_MOD            # a second one behind it: the LOWEST index is reported
    return d


def effective_draws(up):
    """what the launch multiplies by: the batch's own copy of the tail holds 1 in place of a draw >= r (include/h2v.h)"""
    d = draws_of(up)
    return None if d is None else [1 if v >= R_MOD else v for v in d]


def zero_below(up, groups, sizes):
    """per group: the proofs in front of its last zero draw have multiplier zero (a zero FIRST draw zeroes nobody)"""
    d = draws_of(up)
    off = group_offsets(up["n"], groups, sizes)
    out = []
    for g in range(len(off) - 1):
        zb = 0
        if d is not None:
            for j in range(off[g + 1] - off[g] - 1, 0, -1):
                if d[off[g] + j] == 0:
                    zb = j
                    break
        out.append(zb)
    return out


def spoil_positions(up, groups, sizes):
    """[(index, kind)] of the proofs the content changes"""
    n, seed, content = up["n"], up["seed"], up["content"]
    if content == "clean":
        return []
    off = group_offsets(n, groups, sizes)
    if content == "two":            # an undecodable point in the first group, a wrong public input in the last
        first = off[0] + seed % (off[1] - off[0])
        last = off[-2] + (seed * 5) % (off[-1] - off[-2])
        return [(first, "point")] + ([(last, "input")] if last != first else [])
    return [((seed * 13) % n, content)]


def pool_index(up, i, size):
    """which proof of its shape's pool stands at position i; alternating draws stand over adjacent duplicated pairs"""
    return (up["seed"] * 7 + (i // 2 if up["draws"] == "alternating" else i)) % size


def spoil(proof, instances, kind):
    """statuses 0 and a failing pairing ("input", "sign"), -4 ("point"), -5 ("eval")"""
    if kind == "input" and instances[0]:
        return proof, [[((int.from_bytes(instances[0][0], "little") + 1) % R_MOD).to_bytes(32, "little")] + list(instances[0][1:])]
    b = bytearray(proof)
    if kind == "input":             # no public input to change: an evaluation's low bit instead
        b[700] ^= 1
    elif kind == "point":
        b[-33] = 0xff               # the second-last opening point: not decodable
    elif kind == "eval":
        b[-96:-64] = b"\xff" * 32   # an evaluation that is no canonical scalar
    elif kind == "sign":
        b[-1] ^= 0x40               # the last opening point: -P
    else:
        raise ValueError(kind)
    return bytes(b), instances


def materialise(up, groups, sizes, pools):
    """-> (proofs, instances) of the upload; pools[shape] = (P, I)"""
    P, I = pools[up["shape"]]
    idx = [pool_index(up, i, len(P)) for i in range(up["n"])]
    proofs, insts = [P[j] for j in idx], [I[j] for j in idx]
    for at, kind in spoil_positions(up, groups, sizes):
        proofs[at], insts[at] = spoil(proofs[at], insts[at], kind)
    return proofs, insts


# ------------------------------------------------------------------ the model
class Model:
    def __init__(self, capacity=CAPACITY):
        self.capacity = capacity
        self.stage, self.groups, self.sizes = EMPTY, 1, None
        self.up, self.pairing, self.fault, self.zero = None, None, None, None
        self.second = None          # the second batch's upload while it is in flight

    def view(self):
        return View(dict(self.up) if self.up else None, self.groups, list(self.sizes) if self.sizes else None, self.pairing, self.fault)

    def offsets(self):
        return group_offsets(self.up["n"], self.groups, self.sizes)

    def fits(self, n):
        return n == sum(self.sizes) if self.sizes is not None else n % self.groups == 0

    def legal_ns(self):
        return [n for n in SIZES if self.fits(n)]

    def refuses(self, call, ranges=None):
        """would `call` be refused now, leaving everything as it is?  (a draw fault's refusal empties the batch: not this)"""
        if call in CONDITIONAL:
            if self.stage not in CONDITIONAL[call]:
                return False
            if call == "finish_grouped":
                return self.groups > 1
            if call == "export_ragged":
                return self.sizes is not None
            if call == "recheck_cross":
                return self.groups > 1
            return any(self.zero)   # recheck_zero, identify_zero
        if self.stage < LEAST[call]:
            return True
        if call == "finish":
            return self.groups > 1
        if call == "export":
            return self.sizes is not None
        if call == "identify":
            return any(self.zero)
        if call == "recheck":
            off = self.offsets()
            for f, c in ranges:
                g = max(k for k in range(len(off) - 1) if off[k] <= f)
                if c < 1 or f + c > off[g + 1] or f - off[g] < self.zero[g]:
                    return True
        return False

    def illegal_now(self):
        """the rows of illegal_table() that can be generated in this state"""
        calls = [c for c, least in LEAST.items() if self.stage < least] + [c for c in CONDITIONAL if self.refuses(c)]
        return [(self.stage, c) for c in calls]

    def apply(self, step):
        """-> Outcome, and the state after the step"""
        op, kw = step.op, step.kw
        ok = lambda: Outcome("ok", 0, self.view())
        refused = lambda: Outcome("refused", BAD_ARGUMENT, self.view())
        if op in ("set_groups", "set_group_sizes"):
            self.groups, self.sizes = (kw["groups"], None) if op == "set_groups" else (len(kw["sizes"]), list(kw["sizes"]))
            self.stage, self.up, self.fault, self.pairing = EMPTY, None, None, None
            return ok()
        if op == "upload":
            assert self.fits(kw["n"]) and kw["n"] <= self.capacity, step
            bad = kw.get("bad_draw")
            if bad is not None and kw["route"] in HOST_ROUTES:      # refused at the upload: the batch holds nothing
                self.stage, self.up, self.fault = EMPTY, None, None
                return Outcome("refused_empty", BAD_ARGUMENT, self.view())
            self.up, self.fault = dict(kw), bad
            self.zero = zero_below(self.up, self.groups, self.sizes)
            self.stage, self.pairing = UPLOADED, None
            if kw["route"] == "upload_launch":
                self.stage, self.pairing = LAUNCHED, bool(kw["pairing"])
            return ok()
        if op == "launch":
            if self.refuses("launch"):
                return refused()
            self.stage, self.pairing = LAUNCHED, bool(kw["pairing"])
            return ok()
        if op in ("finish", "finish_groups"):
            if self.refuses(op):
                return refused()
            if self.fault is not None:                              # the deferred draw fault: reported here, the batch left Empty
                v = self.view()
                self.stage, self.up, self.fault = EMPTY, None, None
                return Outcome("refused_empty", BAD_ARGUMENT, v)
            self.stage = FINISHED
            return ok()
        if op in ("finish_into", "export", "identify", "process_batch"):
            return refused() if self.refuses(op) else ok()
        if op == "recheck":
            return refused() if self.refuses(op, kw["ranges"]) else ok()
        if op == "illegal":
            assert (self.stage, kw["call"]) in self.illegal_now(), (STAGE_NAMES[self.stage], step)
            return refused()
        if op == "ctx_call":
            return ok()
        if op == "second_start":
            self.second = dict(kw)
            return ok()
        if op == "second_finish":
            assert self.second is not None
            kw, self.second = self.second, None
            return Outcome("ok", 0, View(second_upload(kw), kw["groups"], None, True, None))
        raise ValueError(op)


def second_upload(kw):
    """the second batch's upload in the first one's terms"""
    return dict(route="upload", n=kw["n"], shape=kw["shape"], draws="random", content=kw["content"], seed=kw["seed"])


def run_model(steps, capacity=CAPACITY):
    """-> [(step, stage before, Outcome)]"""
    m, out = Model(capacity), []
    for s in steps:
        before = m.stage
        out.append((s, before, m.apply(s)))
    return out


# ------------------------------------------------------------------ the generator
ILLEGAL_SHARE, FAILING_SHARE = 0.30, 0.21     # of the legal candidates' weight: about 15 % and 10 % of the steps, with the forced steps between


def _pick(rnd, weighted):
    total = sum(w for w, _ in weighted)
    x = rnd.random() * total
    for w, v in weighted:
        x -= w
        if x < 0:
            return v
    return weighted[-1][1]


def n_class(n):
    return 0 if n <= 64 else (1 if n <= 256 else 2)


class _Generator:
    def __init__(self, seed, focus):
        assert focus is None or focus in FOCUSES, focus
        self.rnd = random.Random("%s/%s" % (seed, focus))
        self.focus, self.m, self.out = focus, Model(), []
        self.queue = []                 # steps already decided (a recovery, a scripted prefix)
        self.seen = collections.Counter()
        self.prev_label, self.prev_route, self.prev_n, self.serial = None, None, None, seed * 100
        self.fails_in_a_row = 0
        self.last_launch_route, self.after_launch, self.after_finish_route = None, False, None
        if focus == "sizes":            # across the 256-proof tile boundary and back: 300 -> 255 -> 257 on one object
            for n in (300, 255, 257):
                self.queue += [self.upload(n=n, route=self.rnd.choice(("upload", "device")), content="clean" if n != 255 else "point"),
                               Step("launch", pairing=True), Step("finish")]

    # --- makers
    def spread(self, key, options, base=None):
        """an option, those this sequence has used least after `key` first"""
        weighted = [((base[o] if base else 1.0) / (1 + self.seen[(key, o)]) ** 2, o) for o in options]
        o = _pick(self.rnd, weighted)
        self.seen[(key, o)] += 1
        return o

    def upload(self, n=None, route=None, content=None, failing=False, draws=None, shape=None):
        m, rnd = self.m, self.rnd
        self.serial += 1
        if route is None:
            base = {r: (3.0 if self.focus == "routes" else 1.0) for r in ROUTES}
            route = self.spread(("route", self.prev_route), ROUTES if not failing else ("upload", "upload_launch", "device"), base)
        if n is None:
            ns = m.legal_ns()
            n = self.spread(("n", n_class(self.prev_n) if self.prev_n else None), ns) if self.focus == "sizes" or rnd.random() < 0.5 else rnd.choice(ns)
        if shape is None:
            shape = rnd.choice(SHAPES) if rnd.random() < 0.6 else 8
        if draws is None:
            kinds = [k for k in DRAWS if (k != "zero_at" or n >= 2)]
            draws = _pick(rnd, [((5.0 if k == "random" else 1.0) * (3.0 if k == "random" and self.focus == "readers" else 1.0), k) for k in kinds])
        if route == "device_os":
            draws = "random"            # (not looked at: the library draws)
        if content is None:
            content = _pick(rnd, [((5.0 if c == "clean" else 1.0), c) for c in CONTENT])
        kw = dict(route=route, n=n, shape=shape, draws=draws, content=content, seed=self.serial)
        if route == "upload_launch":
            kw["pairing"] = rnd.random() < 0.8
        if failing:
            kw["draws"] = "random"
            kw["bad_draw"] = rnd.randrange(n)
        return Step("upload", **kw)

    def configure(self):
        """equal -> ragged, ragged -> equal, more groups, fewer groups: the transitions this sequence has made least first"""
        m, rnd = self.m, self.rnd
        if m.sizes is not None:
            kinds = ["ragged->equal", "ragged->ragged"]
        else:
            kinds = ["equal->ragged"] + (["up"] if m.groups < GROUPS[-1] else []) + (["down"] if m.groups > GROUPS[0] else [])
        want = self.spread("configure", kinds, {"ragged->equal": 2.0, "ragged->ragged": 1.0, "equal->ragged": 1.0, "up": 1.0, "down": 1.0})
        if want == "ragged->ragged":   # (mostly the same count and sum: only the sizes change, and the offsets on the device with them)
            same = [s for s in RAGGED if s != m.sizes and len(s) == len(m.sizes) and sum(s) == sum(m.sizes)]
            return Step("set_group_sizes", sizes=list(rnd.choice(same if same and rnd.random() < 0.7 else [s for s in RAGGED if s != m.sizes])))
        if want == "equal->ragged":
            return Step("set_group_sizes", sizes=list(rnd.choice(RAGGED)))
        if want == "ragged->equal":
            return Step("set_groups", groups=rnd.choice(GROUPS))
        return Step("set_groups", groups=rnd.choice([g for g in GROUPS if (g > m.groups) == (want == "up") and g != m.groups]))

    def ranges(self):
        """up to three legal ranges: what a group's non-zero multipliers cover, a single proof, a group's last proof"""
        m, rnd = self.m, self.rnd
        off, out = m.offsets(), []
        for _ in range(rnd.randrange(1, 4)):
            g = rnd.randrange(len(off) - 1)
            lo, hi = off[g] + m.zero[g], off[g + 1]
            kind = rnd.randrange(3)
            if kind == 0:
                out.append((lo, hi - lo))
            elif kind == 1:
                f = rnd.randrange(lo, hi)
                out.append((f, rnd.randrange(1, min(hi - f, 70) + 1)))
            else:
                out.append((hi - 1, 1))
        return out

    def reader(self, name):
        rnd = self.rnd
        if name == "recheck":
            return Step("recheck", ranges=self.ranges())
        if name == "finish_into":
            if rnd.random() < 0.5:
                return Step("finish_into", outputs=list(OUTPUTS), cap=None)
            some = [o for o in OUTPUTS if rnd.random() < 0.5] or ["summary"]
            return Step("finish_into", outputs=some, cap=rnd.choice((1, 2, 5)))
        return Step(name)

    def readers_now(self):
        m = self.m
        names = []
        for r in READERS:
            if r == "recheck":
                if m.stage == FINISHED:
                    names.append(r)
            elif r == "identify":
                # (a single proof's check equals SingleStrategy's only under random draws: programmed draws can cancel two bad proofs)
                if not m.refuses(r) and (m.up["draws"] == "random") and m.fault is None:
                    names.append(r)
            elif not m.refuses(r):
                names.append(r)
        return names

    def first_reader(self, names):
        """directly behind a launch: every reader behind every route's launch; finish_groups behind a launch without a pairing"""
        if self.m.pairing is False and self.rnd.random() < 0.5:
            return "finish_groups"
        return self.spread(("after_launch", self.last_launch_route), names)

    def next_reader(self, names):
        """on a finished launch: the readers that need one directly behind the finish of every route's launch, then every reader behind every other"""
        if self.after_finish_route is not None:
            late = [r for r in names if LEAST[r] == FINISHED]
            if late and self.rnd.random() < 0.8:
                return self.spread(("after_finish", self.after_finish_route), late)
        return self.spread(("reader", self.prev_label), [r for r in names if r != self.prev_label or self.rnd.random() < 0.2] or names)

    def illegal(self):
        rows = self.m.illegal_now()
        if not rows:
            return None
        row = self.spread("illegal", rows, {r: (3.0 if r[1] in CONDITIONAL else 1.0) for r in rows})   # (the rarer ones first)
        return Step("illegal", call=row[1])

    def ctx_call(self):
        self.serial += 1
        other = [s for s in SHAPES if not self.m.up or s != self.m.up["shape"]]
        return Step("ctx_call", kind=self.spread("ctx", CTX_KINDS), shape=self.rnd.choice(other), seed=self.serial)

    def second(self):
        self.serial += 1
        if self.m.second is None:
            return Step("second_start", n=self.rnd.choice((24, 65)), shape=self.rnd.choice(SHAPES), groups=1, content=self.rnd.choice(("clean", "sign", "point")),
                        seed=self.serial)
        return Step("second_finish")

    # --- the choice
    def choose(self):
        m, rnd, focus = self.m, self.rnd, self.focus
        cand = []
        add = lambda w, make: cand.append((w, make))
        if m.stage == EMPTY:
            add({"groups": 5.0, "readers": 0.5, "routes": 0.5}.get(focus, 2.0), self.configure)
            add(8.0, self.upload)
        elif m.stage == UPLOADED:
            add(12.0, lambda: Step("launch", pairing=rnd.random() < 0.75))
            add(0.7, self.upload)
        else:
            names = self.readers_now()
            if m.stage == LAUNCHED:
                add(12.0, lambda: self.reader(self.first_reader(names)))
                add(1.2, lambda: Step("launch", pairing=rnd.random() < 0.75))
                add(0.4, self.upload)
            else:
                add(9.0 if focus != "readers" else 30.0, lambda: self.reader(self.next_reader(names)))
                add(1.8, lambda: Step("launch", pairing=rnd.random() < 0.6))
                add({"routes": 12.0, "sizes": 8.0}.get(focus, 4.0), self.upload)
                add({"groups": 5.0, "readers": 0.3, "routes": 0.4}.get(focus, 1.5), self.configure)
        legal = sum(w for w, _ in cand)
        add(legal * (0.06 if focus != "context" else 0.25), self.ctx_call)
        add(legal * (0.05 if focus != "context" else 0.25) * (5.0 if m.second is not None else 1.0), self.second)
        if self.fails_in_a_row < 2:
            total = sum(w for w, _ in cand)
            if m.illegal_now():     # (the stages a sequence spends least time in get more of them)
                add(total * ILLEGAL_SHARE * (2.5 if m.stage <= UPLOADED else 1.0), self.illegal)
            add(total * FAILING_SHARE, lambda: self.upload(failing=True))
        while True:
            step = _pick(rnd, cand)()
            if step is not None:
                return step

    def recovery(self, deferred):
        """after a failing upload: (an illegal call on the empty batch,) a successful upload, its launch and a full read"""
        steps = []
        if deferred:    # the fault of a device upload comes with the finish: launch, (a device finish that names it,) the refusal
            steps += [Step("launch", pairing=True)]
            if self.rnd.random() < 0.6:
                steps += [Step("finish_into", outputs=list(OUTPUTS), cap=None)]
            steps += [Step("finish_groups")]
        up = self.upload(content=self.rnd.choice(("clean", "clean", "input", "two")))
        steps += [up]
        if up.kw["route"] != "upload_launch":
            steps += [Step("launch", pairing=True)]
        return steps + [Step("finish_groups")]

    def run(self, steps):
        while len(self.out) < steps:
            step = self.queue.pop(0) if self.queue else self.choose()
            sizes_before = self.m.sizes
            outcome = self.m.apply(step)
            self.out.append(step)
            failed = outcome.kind != "ok"
            self.fails_in_a_row = self.fails_in_a_row + 1 if failed else 0
            if step.op == "set_group_sizes" and sizes_before is not None and sizes_before != step.kw["sizes"] and not self.queue and \
                    (len(sizes_before), sum(sizes_before)) == (len(step.kw["sizes"]), sum(step.kw["sizes"])):
                # only the sizes changed: the offsets on the device are h2v_batch_set_group_sizes' own copy, and only an upload from device
                # memory relies on it — with known draws, a pairing and failures in the first and the last group, everything that reads them shows
                self.queue = [self.upload(route="device", draws="random", content="two"), Step("launch", pairing=True),
                              Step("finish_into", outputs=list(OUTPUTS), cap=None), Step("finish_groups")]
            if step.op == "upload":
                if step.kw.get("bad_draw") is not None and not self.queue:
                    self.queue = self.recovery(deferred=not failed)
                    if failed and self.rnd.random() < 0.5 and self.fails_in_a_row < 2:
                        ill = self.illegal()
                        if ill is not None:
                            self.queue.insert(0, ill)
                if not failed and step.kw.get("bad_draw") is None:
                    self.prev_route, self.prev_n = step.kw["route"], step.kw["n"]
                if not failed and step.kw["route"] == "upload_launch":
                    self.last_launch_route = "upload_launch"
            if step.op == "launch" and not failed:
                self.last_launch_route = self.m.up["route"]
            launched = not failed and (step.op == "launch" or (step.op == "upload" and step.kw["route"] == "upload_launch"))
            self.after_finish_route = self.last_launch_route if (self.after_launch and not failed and step.op in ("finish", "finish_groups")) else None
            self.after_launch = launched
            self.prev_label = step.op if (not failed and step.op in READERS) else None
        return self.out


def sequence(seed, steps, focus=None):
    """`steps` steps from `seed`: legal calls by weight, about 15 % calls the stage refuses, about 10 % failing uploads (each followed
    by a successful upload and a full read), never more than two failures in a row; `focus` biases toward one family of FOCUSES"""
    return _Generator(seed, focus).run(steps)


# Above the capacity of the generated sequences: h2v_batch_upload_launch copies the point bytes first and decompresses under the copy of
# the rest only from 2048 proofs on (csrc/batch.hip upload_impl, `points_first`), and only then is `decompressed` set — the flag that lets
# the launch skip the decompression and fill only fold_failed's words.  One scripted sequence on a Batch of LARGE_CAPACITY proofs puts
# every other route behind such an upload, and such an upload behind itself and a relaunch.
LARGE_CAPACITY = 2048


def large_sequence():
    up = lambda route, content, seed, **kw: Step("upload", route=route, n=LARGE_CAPACITY, shape=8, draws="random", content=content, seed=seed, **kw)
    return [up("upload_launch", "clean", 9001, pairing=True), Step("finish"),
            up("device", "two", 9002), Step("launch", pairing=True), Step("finish_groups"), Step("finish_into", outputs=list(OUTPUTS), cap=None),
            up("upload_launch", "point", 9003, pairing=True), Step("finish_groups"), Step("launch", pairing=True), Step("finish"),
            up("upload_launch", "sign", 9004, pairing=False), Step("export"),
            up("upload", "eval", 9005), Step("launch", pairing=True), Step("finish"), Step("recheck", ranges=[(0, 2048), (2047, 1), (1000, 70)]),
            up("upload_launch", "clean", 9006, pairing=True), up("device_os", "input", 9007), Step("launch", pairing=True), Step("finish_groups"),
            Step("set_groups", groups=4),
            up("upload_launch", "two", 9008, pairing=True), Step("finish_groups"), Step("process_batch"),
            up("device", "clean", 9009), Step("launch", pairing=False), Step("finish_into", outputs=["status", "group_failed", "summary"], cap=2), Step("finish_groups")]


# the committed cases: (seed, focus, steps).  tests/test_batch_sequence_host.py asserts what they cover together.
CASES = (
    (93, "groups", 40), (60, "routes", 40), (10, "readers", 40), (144, "groups", 40), (158, "readers", 40), (148, "readers", 40), (198, "sizes", 40),
    (4, "groups", 40), (23, "groups", 40), (28, "context", 40), (118, "context", 40), (7, "routes", 40), (2, "readers", 40), (3, "groups", 40),
)
SHUFFLED = (4, 9, 1, 12, 7, 11, 13, 2, 10, 5, 0, 8, 6, 3)     # the order of the run that reuses one Batch for all of them


# ------------------------------------------------------------------ the expected values (references only)
class Expect:
    """What every successful step returns, from the references: pools[shape] = (proofs, instances) of one circuits.Setup."""

    def __init__(self, setup, pools):
        self.setup, self.pools = setup, pools
        self._launch, self._each = {}, {}

    def items(self, view):
        P, I = materialise(view.up, view.groups, view.sizes, self.pools)
        return [(self.setup, p, i) for p, i in zip(P, I)]

    def each(self, item):
        """verify_each's status of one proof (SingleStrategy), cached"""
        import circuits
        key = batch_reference._key(*item)
        if key not in self._each:
            self._each[key] = circuits.oracle_verify_single(*item)
        return self._each[key]

    def launch(self, view):
        """-> dict(statuses, left[G], right[G], pair[G]) of the launch; left / right / pair None under OS draws"""
        import circuits
        key = (tuple(sorted(view.up.items())), view.groups, tuple(view.sizes) if view.sizes else None)
        hit = self._launch.get(key)
        if hit is None:
            items, draws = self.items(view), effective_draws(view.up)
            off = group_offsets(view.up["n"], view.groups, view.sizes)
            hit = dict(statuses=[batch_reference.single(*it)[0] for it in items], left=None, right=None, pair=None, off=off)
            if draws is not None:
                hit["left"], hit["right"], hit["pair"] = [], [], []
                for g in range(len(off) - 1):
                    _, st, left, right = batch_reference.expected(items[off[g]:off[g + 1]], draws[off[g]:off[g + 1]])
                    assert st == hit["statuses"][off[g]:off[g + 1]]
                    hit["left"].append(left); hit["right"].append(right)
                    hit["pair"].append(circuits.oracle_pairing_check(self.setup, left, right))
            else:   # every proof that SingleStrategy accepts: the group's pairing passes; one that it rejects with status 0: it fails (2^-254)
                hit["pair"] = [all(self.each(it) == 0 or batch_reference.single(*it)[0] != 0 for it in items[off[g]:off[g + 1]]) for g in range(len(off) - 1)]
            self._launch[key] = hit
        return hit

    def group_ok(self, view):
        r = self.launch(view)
        off, st = r["off"], r["statuses"]
        return [not any(st[off[g]:off[g + 1]]) and (r["pair"][g] or not view.pairing) for g in range(len(off) - 1)]

    def finish_groups(self, view):
        r = self.launch(view)
        return self.group_ok(view), r["statuses"], r["left"], r["right"]

    def finish_into(self, view, cap):
        """the seven outputs (tests/results_reference.py over the launch's statuses and verdicts)"""
        import results_reference as rr
        r = self.launch(view)
        G = len(r["off"]) - 1
        fault = rr.NO_FAULT if view.fault is None else view.fault
        oks = [int(v) if view.fault is None else 0 for v in self.group_ok(view)]
        st = r["statuses"]
        return {"status": st, "group_ok": oks, "left_xy": r["left"], "right_xy": r["right"],
                "group_failed": rr.group_failed(st, view.groups, view.sizes), "failed_index": rr.failed_index(st, cap),
                "summary": rr.summary(st, oks, G, rr.FLAG_PAIRING if view.pairing else 0, fault)}

    def recheck(self, view, ranges):
        """-> (oks, lefts, rights); lefts / rights None under OS draws"""
        r = self.launch(view)
        items, draws, off = self.items(view), effective_draws(view.up), r["off"]
        oks, lefts, rights = [], [], []
        for f, c in ranges:
            g = max(k for k in range(len(off) - 1) if off[k] <= f)
            if draws is None:
                oks.append(all(self.each(it) == 0 or batch_reference.single(*it)[0] != 0 for it in items[f:f + c]))
                continue
            ok, left, right = batch_reference.expected_range(items[off[g]:off[g + 1]], draws[off[g]:off[g + 1]], f - off[g], c)
            oks.append(ok); lefts.append(left); rights.append(right)
        return (oks, lefts, rights) if draws is not None else (oks, None, None)

    def identify(self, view):
        """-> (statuses as verify_each returns them, group_own_ok)"""
        r = self.launch(view)
        return [self.each(it) for it in self.items(view)], list(r["pair"])

    def process_batch(self, view):
        """a fresh accumulator fed the batch -> ((n, failed), read(), finalize()); the points None under OS draws"""
        r = self.launch(view)
        n, failed = view.up["n"], sum(1 for v in r["statuses"] if v)
        draws = effective_draws(view.up)
        if draws is None:
            return (n, failed), (None, None, n, failed), (not failed and all(r["pair"]), None, None)
        ok, _, left, right = batch_reference.expected(self.items(view), draws)     # ONE accumulation over all groups' proofs and draws
        return (n, failed), (left, right, n, failed), (ok, left, right)

    def export(self, view):
        """per group: (failed, left point, right point), the points affine (None = the identity) or absent under OS draws"""
        import record_reference
        r = self.launch(view)
        off, st = r["off"], r["statuses"]
        pt = lambda b: record_reference.point_from_bytes(b)[0]
        return [(sum(1 for v in st[off[g]:off[g + 1]] if v), pt(r["left"][g]) if r["left"] else None, pt(r["right"][g]) if r["right"] else None)
                for g in range(len(off) - 1)]

    # --- the one-shot calls
    def ctx_inputs(self, kind, shape, seed):
        """the arguments of a context call, from plain data"""
        rnd = random.Random(7000 + seed)
        P, I = self.pools[shape]
        if kind in ("verify_batch", "verify_each", "verify_batch_identify"):
            n = {"verify_batch": 3 + seed % 4, "verify_each": 4, "verify_batch_identify": 6}[kind]
            idx = [(seed + i) % len(P) for i in range(n)]
            proofs, insts = [P[j] for j in idx], [I[j] for j in idx]
            if kind != "verify_batch" or seed % 2:
                proofs[1], insts[1] = spoil(proofs[1], insts[1], "sign" if kind != "verify_each" else "input")
            return proofs, insts, [rnd.randrange(1, R_MOD) for _ in range(n)]
        if kind == "guard_msm":
            return P[seed % len(P)], I[seed % len(P)]
        import circuits
        rc, g = circuits.oracle_guard(self.setup, self.pools[8][0][0], self.pools[8][1][0])     # a list of points on the curve
        assert rc == 0
        bases = [b for b in g["right_bases"] if any(b)]
        if kind == "msm_g1":
            sc = [0, 1, R_MOD - 1] + [rnd.randrange(R_MOD) for _ in range(297)]
            return sc, [bases[i % len(bases)] for i in range(300)]
        return [([rnd.randrange(R_MOD) for _ in range(k)], [bases[(seed + i) % len(bases)] for i in range(k)]) for k in (5, 9)]   # eval_many

    def ctx_call(self, kind, shape, seed):
        import circuits
        import oracle_lib
        args = self.ctx_inputs(kind, shape, seed)
        if kind in ("verify_batch", "verify_batch_identify"):
            proofs, insts, rand = args
            items = [(self.setup, p, i) for p, i in zip(proofs, insts)]
            ok, st, left, right = batch_reference.expected(items, rand)
            return (ok, st if kind == "verify_batch" else [self.each(it) for it in items], left, right)
        if kind == "verify_each":
            return [self.each((self.setup, p, i)) for p, i in zip(args[0], args[1])]
        if kind == "guard_msm":
            return circuits.oracle_guard(self.setup, *args)
        if kind == "msm_g1":
            return oracle_lib.g1_msm(self.setup.L, *args)
        return [oracle_lib.g1_msm(self.setup.L, sc, bs) for sc, bs in args]
