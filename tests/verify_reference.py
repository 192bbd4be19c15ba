"""Plain big-integer references of what a proof goes through before the MSM (halo2_verifier_amd/csrc/verify_kernels.hip), written from
the reference's definitions — transcript/mod.rs:124-272,484-515, lib.rs:173-218, poly/domain.rs:187-212 — and not from the kernels, and the
programmed inputs that tests/test_gpu_verify_units.py runs through build/verify_units.  tests/test_verify_reference.py holds the
references against the oracle library on the same inputs, so they are not merely self-consistent.  TEST INFRASTRUCTURE ONLY."""
import hashlib
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import pyref  # noqa: E402

P, R = pyref.P, pyref.R
# the project's cube root of unity in Fq (csrc/curve.hip.h: g1_beta_times): phi(x, y) = (beta x, y)
BETA = 0x30644e72e131a0295e6dd9e7e0acccb0c28f069fbb966e3de4bd44e5607cfd48
assert BETA != 1 and pow(BETA, 3, P) == 1, "beta is a primitive cube root of unity"

# the device's rank-coded status words (csrc/batch.h): the smallest wins
ST_INVALID_INSTANCES, ST_TRANSCRIPT, ST_PANIC, ST_OPENING = -40, -30, -20, -10


def le32(v):
    return int(v).to_bytes(32, "little")


# ------------------------------------------------------------------ G1Affine::from_bytes + what the transcript absorbs (mod.rs:158-166, 216-231)
def g1_decode(b):
    """32 compressed bytes -> (x, y), or None where reading the point is an error: x >= p under the 254-bit mask, x^3 + 3 a non-residue,
    or the identity's flag — the identity may decode, but it cannot be absorbed, so the read fails either way."""
    assert len(b) == 32
    v = int.from_bytes(b, "little")
    x = v & ((1 << 254) - 1)
    if x >= P or b[31] & 0x80:
        return None
    rhs = (x * x * x + 3) % P
    y = pow(rhs, (P + 1) // 4, P)
    if y * y % P != rhs:
        return None
    if (y & 1) != (b[31] >> 6) & 1:
        y = (P - y) % P
    return (x, y)


def phi(pt):
    return (BETA * pt[0] % P, pt[1])


def fr_canonical(b):
    """Fr::from_repr accepts these 32 bytes"""
    return int.from_bytes(b, "little") < R


def decompress_expect(proofs, inst, point_offsets, scalar_offsets, n_main, ninst):
    """per proof: ([(x, y) or None per point slot], the status word after the decompression and the scalar check).  The earliest step
    of the reference's sequence wins: instance values are typed Fr before the call, then the main transcript's reads (points and
    scalars), then the multi-open part's points."""
    out = []
    for p, proof in enumerate(proofs):
        pts = [g1_decode(proof[o:o + 32]) for o in point_offsets]
        st = 0
        if any(q is None for q in pts[n_main:]): st = ST_OPENING
        if any(q is None for q in pts[:n_main]) or any(not fr_canonical(proof[o:o + 32]) for o in scalar_offsets): st = ST_TRANSCRIPT
        if any(not fr_canonical(inst[p][32 * i:32 * i + 32]) for i in range(ninst)): st = ST_INVALID_INSTANCES
        out.append((pts, st))
    return out


# ------------------------------------------------------------------ the absorbed stream: a TranscriptSrc table byte for byte (csrc/vkplan.h)
CONST, PROOF, PROOF_MASKED, YCOORD, INSTANCE = range(5)


def absorbed_stream(table, proof, ycanon, inst):
    """table: [(kind, value, offset)] -> the bytes one proof's transcript absorbs"""
    src = {PROOF: proof, PROOF_MASKED: proof, YCOORD: ycanon, INSTANCE: inst}
    out = bytearray()
    for kind, value, off in table:
        if kind == CONST: out.append(value)
        elif kind == PROOF_MASKED: out.append(src[kind][off] & 0x3f)    # the x coordinate without the point's two flag bits
        else: out.append(src[kind][off])
    return bytes(out)


def stream_words(stream_len, keccak):
    """64-bit words per proof in the words buffer: whole hash blocks plus room for a final partial one (csrc/batch.h)"""
    bw = 17 if keccak else 16
    return ((stream_len + 7) // 8 + bw) // bw * bw


def challenges(stream, squeeze_at, keccak):
    """challenge q = the digest of the first squeeze_at[q] absorbed bytes, 64 bytes little-endian mod r (mod.rs:209-214, 239-254, 500-514)"""
    out = []
    for L in squeeze_at:
        if keccak: wide = pyref.keccak256(stream[:L] + b"\x0a") + pyref.keccak256(stream[:L] + b"\x0b")
        else: wide = hashlib.blake2b(stream[:L], digest_size=64, person=b"Halo2-Transcript").digest()
        out.append(int.from_bytes(wide, "little") % R)
    return out


# ------------------------------------------------------------------ instance evaluation (lib.rs:173-218, poly/domain.rs:187-212)
def omega_of(k):
    """the 2^k-th root of unity, from the project's ROOT_OF_UNITY (oracle/pyref.py)"""
    w = pyref.ROOT_OF_UNITY
    for _ in range(pyref.S - k): w = w * w % R
    return w


def batch_inverse(v):
    """1 / v[i] mod r for non-zero v[i]"""
    pre, run = [], 1
    for x in v:
        pre.append(run); run = run * x % R
    inv = pow(run, -1, R)
    out = [0] * len(v)
    for i in range(len(v) - 1, -1, -1):
        out[i] = inv * pre[i] % R
        inv = inv * v[i] % R
    return out


def instance_eval(vals, rot, x, k):
    """sum_j a_j l_{j - rot}(x) with l_i(x) = omega^i (x^n - 1) / (n (x - omega^i)); a value that is no canonical Fr counts as zero.
    None where a denominator is zero: x lies on the domain (the project reports it as a reference panic)."""
    n, w = 1 << k, omega_of(k)
    wi, pows = pow(w, -rot % n, R), []
    for _ in vals:
        pows.append(wi); wi = wi * w % R
    den = [(x - wp) % R for wp in pows]
    if 0 in den: return None
    common = (pow(x, n, R) - 1) * pow(n, -1, R) % R
    acc = 0
    for a, wp, di in zip(vals, pows, batch_inverse(den)):
        if a < R: acc = (acc + a * wp % R * di) % R
    return acc * common % R


# ------------------------------------------------------------------ the Fr program (csrc/vkplan.h: VmOp)
(OP_CONST, OP_MUL, OP_ADD, OP_SUB, OP_NEG, OP_INV, OP_POW, OP_SQRN, OP_LOAD_SCALAR, OP_LOAD_INST, OP_LOAD_CHAL, OP_LOAD_MULT, OP_STORE_MSM,
 OP_STORE_SHARED, OP_STORE_LEFT, OP_LOAD_INSTEVAL, OP_STORE_GUARD, OP_BARRIER) = range(1, 19)
VM_CONST_OPERAND = 0x80000000
FILL = int.from_bytes(b"\x11" * 32, "little")     # what the harness leaves in a row no store wrote
WRITES = {OP_CONST, OP_MUL, OP_ADD, OP_SUB, OP_NEG, OP_INV, OP_POW, OP_SQRN, OP_LOAD_SCALAR, OP_LOAD_INST, OP_LOAD_CHAL, OP_LOAD_MULT, OP_LOAD_INSTEVAL}


class VmEnv:
    """one proof's inputs: scalars / inst as canonical-or-not 256-bit integers (a non-canonical one loads as zero), the rest residues"""
    def __init__(self, scalars, inst, chal, insteval, mult, status=0):
        self.scalars, self.inst, self.chal, self.insteval, self.mult, self.status = scalars, inst, chal, insteval, mult, status


def vm_run(code, consts, env, np, n_guard, n_shared):
    """interpret `code` (a list of (op, d, a, b)) for one proof -> dict(msm, left, guard, shared, status).  A store of the MSM, left
    and shared channels is zero once the proof's status is non-zero; the Guard's is not.  Reading a slot nothing wrote is an error of
    the program, not of the proof: it raises."""
    slots, st = {}, env.status
    out = dict(msm=[FILL] * np, left=[FILL] * np, guard=[FILL] * n_guard, shared=[None] * n_shared)
    opnd = lambda x: consts[x & ~VM_CONST_OPERAND] if x & VM_CONST_OPERAND else slots[x]
    load = lambda v: v if v < R else 0
    for op, d, a, b in code:
        if op == OP_BARRIER: continue
        elif op == OP_CONST: v = consts[a]
        elif op == OP_MUL: v = opnd(a) * opnd(b) % R
        elif op == OP_ADD: v = (opnd(a) + opnd(b)) % R
        elif op == OP_SUB: v = (opnd(a) - opnd(b)) % R
        elif op == OP_NEG: v = -slots[a] % R
        elif op == OP_INV:
            if slots[a] == 0: st = min(st, ST_PANIC)
            v = pow(slots[a], R - 2, R)          # (the inverse of zero is zero)
        elif op == OP_POW: v = pow(slots[a], b, R)
        elif op == OP_SQRN: v = pow(slots[a], 1 << b, R)
        elif op == OP_LOAD_SCALAR: v = load(env.scalars[a])
        elif op == OP_LOAD_INST: v = load(env.inst[a])
        elif op == OP_LOAD_CHAL: v = env.chal[a]
        elif op == OP_LOAD_INSTEVAL: v = env.insteval[a]
        elif op == OP_LOAD_MULT: v = env.mult
        elif op == OP_STORE_MSM: out["msm"][b] = 0 if st else slots[a]; continue
        elif op == OP_STORE_LEFT: out["left"][b] = 0 if st else slots[a]; continue
        elif op == OP_STORE_SHARED: out["shared"][b] = 0 if st else slots[a]; continue
        elif op == OP_STORE_GUARD: out["guard"][b] = slots[a]; continue
        else: raise ValueError(op)
        slots[d] = v
    out["status"] = st
    return out


def vm_split(code, K, n_slots):
    """the program as K instruction streams that meet at barriers, under the interpreter's contract — a stream reads a slot another
    stream wrote only behind a barrier: the program is cut into segments at its barriers, and inside a segment instruction i goes to
    the stream of the first instruction (of that segment) that wrote one of its operands, or that reads or overwrites the slot it
    writes; an instruction tied to nothing goes round robin.  Every stream gets every barrier.  The streams together hold the
    program's instructions once, in program order, so they compute what the single stream computes."""
    streams = [[] for _ in range(K)]
    owner, rr = {}, 0
    st_writer, st_readers = None, set()      # the status word: OP_INV may set it, the zeroing stores read it
    zeroing = (OP_STORE_MSM, OP_STORE_LEFT, OP_STORE_SHARED)
    def barrier():
        nonlocal owner, st_writer, st_readers
        for s in streams: s.append((OP_BARRIER, 0, 0, 0))
        owner, st_writer, st_readers = {}, None, set()
    for ins in code:
        op, d, a, b = ins
        if op == OP_BARRIER:
            barrier()
            continue
        reads = []
        if op in (OP_MUL, OP_ADD, OP_SUB): reads = [x for x in (a, b) if not x & VM_CONST_OPERAND]
        elif op in (OP_NEG, OP_INV, OP_POW, OP_SQRN, OP_STORE_MSM, OP_STORE_LEFT, OP_STORE_SHARED, OP_STORE_GUARD): reads = [a]
        touched = reads + ([d] if op in WRITES else [])
        tied = {owner[s] for s in touched if s in owner}
        if op in zeroing and st_writer is not None: tied.add(st_writer)
        if op == OP_INV: tied |= st_readers | ({st_writer} if st_writer is not None else set())
        if len(tied) > 1:
            # it joins what two streams did in this segment: close the segment in front of it
            barrier()
            tied = set()
        if tied: w = min(tied)
        else: w = rr % K; rr += 1
        streams[w].append(ins)
        for s in touched: owner[s] = w
        if op in zeroing: st_readers.add(w)
        if op == OP_INV: st_writer = w
    for s in streams:
        if not s: s.append((OP_BARRIER, 0, 0, 0))
    nb = max(sum(1 for i in s if i[0] == OP_BARRIER) for s in streams)
    for s in streams:
        s.extend([(OP_BARRIER, 0, 0, 0)] * (nb - sum(1 for i in s if i[0] == OP_BARRIER)))
    return streams


def vm_random_program(rnd, n_slots, length, sizes, with_inv=True):
    """a seeded program that respects the interpreter's contract: a slot is read only after it was written.  sizes = dict(consts, ns,
    ninst, n_chal, n_insteval, np, n_guard, n_shared).  Every output row is stored at the end, after a barrier."""
    code, written = [], []
    def dst():
        d = rnd.randrange(n_slots)
        if d in written: written.remove(d)
        written.append(d)
        return d
    def src():
        # the previous result, the one before it, or any written slot
        r = rnd.random()
        if r < 0.3: return written[-1]
        if r < 0.45 and len(written) > 1: return written[-2]
        return rnd.choice(written)
    loads = [(OP_CONST, sizes["consts"]), (OP_LOAD_SCALAR, sizes["ns"]), (OP_LOAD_INST, sizes["ninst"]), (OP_LOAD_CHAL, sizes["n_chal"]),
             (OP_LOAD_INSTEVAL, sizes["n_insteval"]), (OP_LOAD_MULT, 1)]
    for op, cnt in loads:
        code.append((op, dst(), rnd.randrange(cnt), 0))
    for _ in range(length):
        r = rnd.random()
        if r < 0.1:
            op, cnt = rnd.choice(loads); code.append((op, dst(), rnd.randrange(cnt), 0)); continue
        if r < 0.15: code.append((OP_BARRIER, 0, 0, 0)); continue
        if r < 0.7:
            op = rnd.choice([OP_MUL, OP_ADD, OP_SUB])
            a = src() if rnd.random() < 0.8 else VM_CONST_OPERAND | rnd.randrange(sizes["consts"])
            b = src() if rnd.random() < 0.8 else VM_CONST_OPERAND | rnd.randrange(sizes["consts"])
            form = rnd.random()
            d = a if form < 0.15 and not a & VM_CONST_OPERAND else (b if form < 0.3 and not b & VM_CONST_OPERAND else None)
            if d is None: d = dst()
            else: written.remove(d); written.append(d)
            code.append((op, d, a, b)); continue
        a = src()
        if r < 0.78: code.append((OP_NEG, dst(), a, 0))
        elif r < 0.86: code.append((OP_POW, dst(), a, rnd.choice([0, 1, 2, 3, 0xffffffff, rnd.randrange(1 << 32)])))
        elif r < 0.94: code.append((OP_SQRN, dst(), a, rnd.choice([0, 1, 2, 28])))
        elif with_inv: code.append((OP_INV, dst(), a, 0))
        else: code.append((OP_NEG, dst(), a, 0))
    code.append((OP_BARRIER, 0, 0, 0))
    for ch, op, cnt in (("msm", OP_STORE_MSM, sizes["np"]), ("left", OP_STORE_LEFT, sizes["np"]), ("guard", OP_STORE_GUARD, sizes["n_guard"]), ("shared", OP_STORE_SHARED, sizes["n_shared"])):
        for b in range(cnt): code.append((op, 0, rnd.choice(written), b))
    return code


# ------------------------------------------------------------------ folds
def fold(shared, n, j, first, count):
    """shared: [row][proof] residues -> the sum of row j over proofs [first, first + count)"""
    return sum(shared[j][first:first + count]) % R


# ================================================================== programmed inputs
def enc_point(x, flags):
    """x (any integer below 2^254) and the two flag bits as the 32 bytes of a proof"""
    b = bytearray(le32(x)); b[31] |= flags; return bytes(b)


def on_curve_x(rnd):
    while True:
        x = rnd.randrange(P)
        if pow((x * x * x + 3) % P, (P - 1) // 2, P) == 1: return x


def point_encodings(rnd):
    """[(name, 32 bytes)]: the encodings the decompression must tell apart"""
    out = []
    for i in range(4):
        x = on_curve_x(rnd)
        out += [(f"valid x, sign 0 #{i}", enc_point(x, 0)), (f"valid x, sign 1 #{i}", enc_point(x, 0x40))]   # both roots of one x: either parity
    for x in (1, 2, 3): out += [(f"x = {x}", enc_point(x, 0)), (f"x = {x}, sign", enc_point(x, 0x40))]      # on the curve
    for x in (4, 10): out += [(f"x = {x}", enc_point(x, 0)), (f"x = {x}, sign", enc_point(x, 0x40))]        # off the curve
    for name, x in (("p", P), ("p + 1", P + 1), ("2^254 - 1", (1 << 254) - 1)):                              # >= p under the 254-bit mask
        out += [(f"x = {name}", enc_point(x, 0)), (f"x = {name}, sign", enc_point(x, 0x40))]
    for fl in (0x80, 0xc0, 0x00, 0x40): out.append((f"x = 0, flags {fl:#x}", enc_point(0, fl)))             # 3 is a non-residue: all errors
    out += [("identity flag, x = 1", enc_point(1, 0x80)), ("identity and sign flags, x = 2", enc_point(2, 0xc0)), ("identity flag, random x", enc_point(on_curve_x(rnd), 0x80))]
    return out


# 0, r - 1, r, r + 1, 2^256 - 1, and two values whose top word is r's while they are below r (the slow path that accepts)
SCALAR_VALUES = [0, R - 1, R, R + 1, (1 << 256) - 1, (R >> 224) << 224, R - (1 << 100)]


class DecompressJob:
    """n proofs of np points and ns scalars each (the record's 32-byte cells in a shuffled order) and ninst instance values"""
    def __init__(self, rnd, n, np, n_main, ns=3, ninst=2, special=True, cuts=None):
        self.n, self.np, self.n_main, self.ns, self.ninst = n, np, n_main, ns, ninst
        cells = list(range(np + ns)); rnd.shuffle(cells)
        self.point_offsets, self.scalar_offsets = [32 * c for c in cells[:np]], [32 * c for c in cells[np:]]
        self.proof_len = 32 * (np + ns)
        self.cuts = cuts or sorted({0, n} | ({n // 3, n // 3 + 1, n - 1} if n >= 3 else set()))
        pts = [[enc_point(on_curve_x(rnd), rnd.choice([0, 0x40])) for _ in range(np)] for _ in range(n)]
        sc = [[le32(rnd.randrange(R)) for _ in range(ns)] for _ in range(n)]
        iv = [[le32(rnd.randrange(R)) for _ in range(ninst)] for _ in range(n)]
        self.names = {}
        if special:
            encs = point_encodings(rnd)
            lanes = rnd.sample(range(n * np), min(len(encs), n * np)) if n * np >= len(encs) else [rnd.randrange(n * np) for _ in encs]
            for (name, e), t in zip(encs, lanes):
                pts[t // np][t % np] = e; self.names[(t // np, t % np)] = name
            for v in SCALAR_VALUES:
                sc[rnd.randrange(n)][rnd.randrange(ns)] = le32(v)
                if rnd.random() < 0.5: iv[rnd.randrange(n)][rnd.randrange(ninst)] = le32(v)
        self.pts, self.sc, self.iv = pts, sc, iv

    def proofs(self):
        out = []
        for p in range(self.n):
            b = bytearray(self.proof_len)
            for o, e in zip(self.point_offsets, self.pts[p]): b[o:o + 32] = e
            for o, e in zip(self.scalar_offsets, self.sc[p]): b[o:o + 32] = e
            out.append(bytes(b))
        return out

    def inst(self):
        return [b"".join(v) for v in self.iv]


def decompress_jobs():
    """np in {1, 3, 7}; n np mod 64 = 0, 1, 63; three workgroups and more; pieces with p0 > 0; and the ranking of several faults in one proof"""
    rnd = random.Random(4101)
    jobs = []
    for np, n_main in ((1, 1), (3, 2), (7, 4)):
        for n in {1: (64, 65, 63), 3: (64, 43, 21), 7: (64, 55, 9)}[np]:
            jobs.append(DecompressJob(rnd, n, np, n_main, cuts=[0, n]))   # one launch over n np lanes
            jobs.append(DecompressJob(rnd, n, np, n_main))               # the same shape in pieces
    jobs.append(DecompressJob(rnd, 65, 1, 0))      # (a single point slot that belongs to the multi-open part)
    # ranking: proof 0 has a bad opening point, a bad main point and a non-canonical instance value; proof 1 the first two; proof 2 the first; proof 3 none
    rk = DecompressJob(rnd, 4, 4, 2, special=False, cuts=[0, 1, 4])
    bad = enc_point(4, 0)
    for p in (0, 1, 2): rk.pts[p][3] = bad
    for p in (0, 1): rk.pts[p][0] = bad
    rk.iv[0][1] = le32(R)
    jobs.append(rk)
    # the same with a non-canonical proof scalar in place of the bad main point
    rk2 = DecompressJob(rnd, 4, 4, 2, special=False, cuts=[0, 3, 4])
    for p in (0, 1, 2): rk2.pts[p][2] = bad
    for p in (0, 1): rk2.sc[p][1] = le32(R + 1)
    rk2.iv[0][0] = le32((1 << 256) - 1)
    jobs.append(rk2)
    return jobs


# ---- TranscriptSrc tables
def contract_table(phase, np, ns, ninst, order, tail):
    """The shape compile_plan emits: 32-byte items of the four data kinds — a point's x (31 proof bytes and the masked flag byte) with
    its canonical y straight behind, a proof scalar, an instance value — each behind a one-byte constant prefix, 0x00 markers between
    some of them.  The first item starts at phase `phase` of a word; `tail` constant bytes end the table."""
    t = [(CONST, 0x30 + i, 0) for i in range((phase if phase else 8) - 1)]
    used = dict(P=0, S=0, I=0)
    for what in order:
        if what == "0": t.append((CONST, 0, 0)); continue
        i = used[what]; used[what] += 1
        if what == "P":
            i %= np
            t.append((CONST, 1, 0))
            t += [(PROOF, 0, 32 * i + j) for j in range(31)] + [(PROOF_MASKED, 0, 32 * i + 31)]
            t += [(YCOORD, 0, 32 * i + j) for j in range(32)]
        elif what == "S":
            i %= ns
            t.append((CONST, 2, 0))
            t += [(PROOF, 0, 32 * (np + i) + j) for j in range(32)]
        else:
            i %= ninst
            t.append((CONST, 2, 0))
            t += [(INSTANCE, 0, 32 * i + j) for j in range(32)]
    return t + [(CONST, 0x51 + i, 0) for i in range(tail)]


def freeform_table(rnd, length, sizes):
    """data runs of 1 to 7 bytes (and a few long ones) from any source at any offset — small offsets often, which the fast path must
    refuse: its shifted load would start in front of the record — with and without constants between them.  sizes: {kind: bytes}"""
    t = []
    while len(t) < length:
        kind = rnd.choice([PROOF, PROOF, YCOORD, INSTANCE])
        run = rnd.choice([1, 2, 3, 4, 5, 6, 7, 1, 2, 3, 9, 16, 33])
        off = rnd.choice([0, 0, 1, 2, 3, 5, 6, 7, rnd.randrange(sizes[kind]), sizes[kind] - run])
        off = max(0, min(off, sizes[kind] - run))
        for j in range(run):
            t.append((PROOF_MASKED if kind == PROOF and j == run - 1 and rnd.random() < 0.3 else kind, 0, off + j))
        for _ in range(rnd.choice([0, 0, 1, 1, 2, 5, 9])): t.append((CONST, rnd.randrange(256), 0))
    return t[:length]


class StreamJob:
    def __init__(self, rnd, n, table, squeeze_at, keccak=False, np=3, ns=2, ninst=2):
        self.n, self.table, self.squeeze_at, self.keccak, self.np, self.ninst = n, table, squeeze_at, keccak, np, ninst
        self.proof_len = 32 * (np + ns)
        # every proof its own random bytes: a wrong per-proof stride shows
        self.proofs = [bytes(rnd.randrange(256) for _ in range(self.proof_len)) for _ in range(n)]
        self.ycanon = [bytes(rnd.randrange(256) for _ in range(32 * np)) for _ in range(n)]
        self.inst = [bytes(rnd.randrange(256) for _ in range(32 * ninst)) for _ in range(n)]

    def streams(self):
        return [absorbed_stream(self.table, self.proofs[p], self.ycanon[p], self.inst[p]) for p in range(self.n)]


def long_table(rnd, length):
    t = contract_table(rnd.randrange(8), 3, 2, 2, "PS0ISP0SIP0PSI0SPSI0PPSI0", 0)
    while len(t) < length: t += contract_table(1, 3, 2, 2, "SIP0", 0)
    return t[:length]


BLAKE_SQUEEZES = [[1, 64, 127, 128, 129, 255, 256, 257, 384, 450],          # ... and the stream's full length (450)
                  [128, 130, 131, 256, 300, 301, 302, 512, 513, 640, 641]]  # two and three inside a block; a block right behind a boundary
KECCAK_SQUEEZES = [[1, 134, 135, 136, 137, 271, 272, 273, 300], [136, 272, 407, 408]]


def transcript_jobs(keccak):
    rnd = random.Random(4202 + keccak)
    jobs = []
    for n in ((1, 63, 64, 65) if keccak else (1, 15, 16, 17, 33)):
        for sq in (KECCAK_SQUEEZES if keccak else BLAKE_SQUEEZES):
            jobs.append(StreamJob(rnd, n, long_table(rnd, sq[-1]), sq, keccak))
    return jobs
