"""The per-proof kernels (csrc/verify_kernels.hip: k_decompress, k_check_scalars, k_stream_build, k_transcript, k_transcript_keccak,
k_instance_eval, k_frvm, k_frvm2, k_fold_shared, k_fold_ranges) stage by stage against the big-integer references of
tests/verify_reference.py.  build/verify_units (tests/cpp/verify_units.hip, built by csrc/Makefile with the library's flags) runs the
library's own launchers on inputs programmed here — encodings, TranscriptSrc tables, squeeze positions, VmInstr programs — instead
of what compile_plan and the oracle's prover happen to produce: squeezes on the hash blocks' boundaries, every alignment of the
stream builder's fast path, the register forwarding and the LDS / global slot boundary of the Fr program, the shadow lanes of
k_frvm2, the zero-denominator path of the instance evaluation, fold ranges of several batches in one grid, and the ranking of several
faults in one proof.  Every comparison is exact, on canonical residues and bytes."""
import random
import struct

import pytest

import units_harness as uh
import verify_reference as vr
from units_harness import Cursor

pytestmark = pytest.mark.gpu

P, R = vr.P, vr.R
FILL32 = b"\x11" * 32
H2V_ERR_UNSUPPORTED = -19


def W(*v):
    return struct.pack(f"<{len(v)}I", *[x & 0xffffffff for x in v])


def _run(mode, jobs, tmp_path):
    """jobs: the encoded jobs -> the program's output bytes"""
    return uh.run("verify_units", [mode], W(len(jobs)) + b"".join(jobs), tmp_path, timeout=300)


# ------------------------------------------------------------------ decompression and scalar check
def _enc_decompress(j):
    return (W(j.n, j.np, j.n_main, j.ns, j.ninst, j.proof_len, len(j.cuts) - 1, *j.cuts) + W(*j.point_offsets) + W(*j.scalar_offsets)
            + b"".join(j.proofs()) + b"".join(j.inst()))


def test_decompress_and_scalar_check(tmp_path):
    jobs = vr.decompress_jobs()
    out = Cursor(_run("decompress", [_enc_decompress(j) for j in jobs], tmp_path))
    seen = set()
    for ji, j in enumerate(jobs):
        want = vr.decompress_expect(j.proofs(), j.inst(), j.point_offsets, j.scalar_offsets, j.n_main, j.ninst)
        for p in range(j.n):
            for s in range(j.np):
                got = dict(x=out.num(), y=out.num(), phi_x=out.num(), phi_y=out.num(), identity=out.word(), ycanon=out.take(32))
                pt = want[p][0][s]
                exp = (dict(x=pt[0], y=pt[1], phi_x=vr.phi(pt)[0], phi_y=pt[1], identity=0, ycanon=vr.le32(pt[1])) if pt is not None
                       else dict(x=0, y=0, phi_x=0, phi_y=0, identity=1, ycanon=bytes(32)))
                name = j.names.get((p, s), "a valid point")
                seen.add((name, pt is None))
                for k in exp:
                    assert got[k] == exp[k], f"job {ji} (n={j.n} np={j.np} pieces {j.cuts}) proof {p} slot {s} ({name}): {k} is {got[k]!r}, not {exp[k]!r}"
        for p in range(j.n):
            st = out.sword()
            assert st == want[p][1], f"job {ji} (n={j.n} np={j.np}) proof {p}: status {st}, not {want[p][1]}"
    out.done()
    # the inputs did what they were programmed for: both verdicts occurred, and the ranking proofs ended where they should
    assert {ok for _, ok in seen} == {True, False}
    rk = vr.decompress_expect(jobs[-2].proofs(), jobs[-2].inst(), jobs[-2].point_offsets, jobs[-2].scalar_offsets, 2, 2)
    assert [st for _, st in rk] == [vr.ST_INVALID_INSTANCES, vr.ST_TRANSCRIPT, vr.ST_OPENING, 0]


# ------------------------------------------------------------------ stream build and transcripts
def _enc_stream(j):
    tab = b"".join(W(k | (v << 8), o) for k, v, o in j.table)
    return (W(j.n, 1 if j.keccak else 0, j.proof_len, j.np, j.ninst, len(j.table), len(j.squeeze_at)) + tab + W(*j.squeeze_at)
            + b"".join(j.proofs) + b"".join(j.ycanon) + b"".join(j.inst))


def _check_stream(jobs, out, what):
    for ji, j in enumerate(jobs):
        rc, sw = out.sword(), out.word()
        assert rc == 0, f"{what} job {ji}: transcript_stage_enqueue returned {rc}"
        assert sw == vr.stream_words(len(j.table), j.keccak), f"{what} job {ji}: {sw} stream words"
        streams = j.streams()
        for p in range(j.n):
            got, exp = out.take(8 * sw), streams[p].ljust(8 * sw, b"\0")
            if got != exp:
                at = next(i for i in range(8 * sw) if got[i] != exp[i])
                raise AssertionError(f"{what} job {ji} (n={j.n}, {len(j.table)} bytes) proof {p}: stream byte {at} (word {at // 8}, entry {j.table[at] if at < len(j.table) else 'padding'}) "
                                     f"is {got[at]:#04x}, not {exp[at]:#04x}")
        want = [vr.challenges(s, j.squeeze_at, j.keccak) for s in streams]
        for q in range(len(j.squeeze_at)):
            for p in range(j.n):
                c = out.num()
                assert c == want[p][q], f"{what} job {ji} (n={j.n}) proof {p}: challenge {q} (squeezed at {j.squeeze_at[q]}) is {c:#x}, not {want[p][q]:#x}"


@pytest.mark.parametrize("n", [1, 7, 8, 9, 17])
def test_stream_build(n, tmp_path):
    rnd = random.Random(4300 + n)
    jobs = []
    for phase in range(8):      # the first item at every phase of a word, so the masked flag byte at every byte of one; a final partial word
        t = vr.contract_table(phase, 3, 2, 2, "P0SIP0PS0IS", 1 + phase % 4)
        jobs.append(vr.StreamJob(rnd, n, t, [len(t)]))
    sizes = {vr.PROOF: 160, vr.YCOORD: 96, vr.INSTANCE: 64}
    for length in (5, 8, 9, 64, 201, 333):
        t = vr.freeform_table(rnd, length, sizes)
        jobs.append(vr.StreamJob(rnd, n, t, [len(t)]))
    # words the fast path must refuse or take at its limits, one after another: a run A of 3 bytes from offset 0 (its shifted load
    # would start 5 bytes in front of the record: off[0] < 8 - la), the same from offset 5 (just allowed), a source change without a
    # constant between, three sources in one word, a run B that ends with its record's last byte, a whole word of one source
    K, Pr, Y, I = vr.CONST, vr.PROOF, vr.YCOORD, vr.INSTANCE
    t = ([(Pr, 0, o) for o in (0, 1, 2)] + [(K, 0xc0 + i, 0) for i in range(5)]
         + [(Y, 0, o) for o in (5, 6, 7)] + [(K, 0xd0 + i, 0) for i in range(5)]
         + [(Pr, 0, o) for o in (3, 4, 5)] + [(Y, 0, o) for o in (0, 1, 2, 3, 4)]
         + [(Pr, 0, 9), (Pr, 0, 10), (Y, 0, 40), (Y, 0, 41), (I, 0, 0), (I, 0, 1), (I, 0, 2), (I, 0, 3)]
         + [(K, 1, 0)] + [(I, 0, o) for o in range(57, 64)]
         + [(vr.PROOF_MASKED if o == 159 else Pr, 0, o) for o in range(152, 160)]
         + [(I, 0, 0)] + [(K, 7, 0)] * 6 + [(Y, 0, 95)])
    jobs.append(vr.StreamJob(rnd, n, t, [len(t)]))
    out = Cursor(_run("stream", [_enc_stream(j) for j in jobs], tmp_path))
    _check_stream(jobs, out, "stream build")
    out.done()


def test_transcript_blake2b(tmp_path):
    jobs = vr.transcript_jobs(False)
    out = Cursor(_run("stream", [_enc_stream(j) for j in jobs], tmp_path))
    _check_stream(jobs, out, "Blake2b")
    out.done()


def test_transcript_keccak(tmp_path):
    jobs = vr.transcript_jobs(True)
    out = Cursor(_run("stream", [_enc_stream(j) for j in jobs], tmp_path))
    _check_stream(jobs, out, "Keccak")
    out.done()


def test_transcript_blake2b_challenge_limit(tmp_path):
    """57 challenges are the most the 60 KB rule admits ((16 17 + 16 57 8) 8 = 60 544 bytes); with 58 the launcher refuses with
    H2V_ERR_UNSUPPORTED and launches nothing: the words and the challenges stay as the harness filled them."""
    rnd = random.Random(4400)
    t = vr.long_table(rnd, 700)
    sq57 = sorted(rnd.sample(range(1, 701), 56)) + [700]
    ok = vr.StreamJob(rnd, 17, t, sq57)
    over = vr.StreamJob(rnd, 17, t, sorted(rnd.sample(range(1, 701), 58)))
    out = Cursor(_run("stream", [_enc_stream(ok), _enc_stream(over)], tmp_path))
    _check_stream([ok], out, "57 challenges")
    rc, sw = out.sword(), out.word()
    assert rc == H2V_ERR_UNSUPPORTED, f"58 challenges: transcript_stage_enqueue returned {rc}"
    words = out.take(8 * sw * over.n)
    touched = [i for i in range(len(words)) if words[i] != 0x11]
    assert not touched, f"58 challenges: refused, but {len(touched)} bytes of the words buffer were written, first at byte {touched[0]} (proof {touched[0] // (8 * sw)})"
    for q in range(58):
        for p in range(over.n):
            assert out.take(32) == out_fill_fr(), f"58 challenges: refused, but challenge {q} of proof {p} was written"
    out.done()


def out_fill_fr():
    """the canonical bytes of an Fr whose nine limbs are 0x11111111 (Montgomery, R = 2^261): what an unwritten element reads as"""
    v = sum(0x11111111 << (29 * i) for i in range(9))
    return vr.le32(v * pow(1 << 261, -1, R) % R)


# ------------------------------------------------------------------ instance evaluation
K_INST = 14


def _inst_job(rnd, length, rot, panic=False):
    n, base = 3, 5
    ninst = base + length + 3                          # the column lies inside a proof's values: base > 0, ninst > base + len
    vals = [[rnd.randrange(R) for _ in range(ninst)] for _ in range(n)]
    for p in range(n):                                  # a column that does not start at value 0; non-canonical values count as zero
        vals[p][base] = rnd.randrange(1, R)
        vals[p][base + rnd.randrange(length)] = rnd.choice([R + 1, R + 5, (1 << 256) - 1])   # (not r itself: reduced, it would be zero too)
    xs = [rnd.randrange(R) for _ in range(n)]           # a different x per proof
    if panic:
        j = length // 2
        xs[1] = pow(vr.omega_of(K_INST), (j - rot) % (1 << K_INST), R)   # a zero denominator in the middle of the column
    return dict(n=n, ninst=ninst, base=base, len=length, rot=rot, vals=vals, xs=xs)


def _enc_inst(j):
    n = j["n"]
    chal = [[(7 + p) % R for p in range(n)], j["xs"]]   # x is challenge 1 of 2
    return (W(n, K_INST, j["ninst"], j["base"], j["len"], j["rot"], 1, 2) + vr.le32(vr.omega_of(K_INST))
            + b"".join(vr.le32(v) for p in range(n) for v in j["vals"][p]) + b"".join(vr.le32(c) for row in chal for c in row))


def _check_inst(jobs, out):
    n_panics = 0
    for ji, j in enumerate(jobs):
        want = [vr.instance_eval(j["vals"][p][j["base"]:j["base"] + j["len"]], j["rot"], j["xs"][p], K_INST) for p in range(j["n"])]
        got = [out.num() for _ in range(j["n"])]
        st = [out.sword() for _ in range(j["n"])]
        for p in range(j["n"]):
            what = f"instance evaluation job {ji} (len={j['len']} rot={j['rot']}) proof {p}"
            if want[p] is None:
                n_panics += 1
                assert st[p] == vr.ST_PANIC, f"{what}: x is on the domain, status {st[p]}"
            else:
                assert st[p] == 0, f"{what}: status {st[p]}"
                assert got[p] == want[p], f"{what}: {got[p]:#x}, not {want[p]:#x}"
    return n_panics


@pytest.mark.parametrize("rot", [0, 1, -1])
def test_instance_eval(rot, tmp_path):
    rnd = random.Random(4500 + rot)
    jobs = [_inst_job(rnd, length, rot) for length in (1, 255, 256, 257, 4095, 4096, 4097, 8193)]
    jobs += [_inst_job(rnd, length, rot, panic=True) for length in (257, 4097)]
    out = Cursor(_run("insteval", [_enc_inst(j) for j in jobs], tmp_path))
    assert _check_inst(jobs, out) == 2
    out.done()


# ------------------------------------------------------------------ Fr program
SIZES = dict(consts=6, ns=3, ninst=2, n_chal=2, n_insteval=1, np=6, n_guard=50, n_shared=4)
N_SLOTS = 12
Z_CONST = 0x1234567890abcdef1234567890abcdef          # consts[4]: challenge 0 of one proof equals it


def _consts(rnd):
    return [0, 1, R - 1, rnd.randrange(R), Z_CONST, rnd.randrange(R)]


def _envs(rnd, n, zero_at=None):
    envs = []
    for p in range(n):
        sc = [rnd.randrange(R) for _ in range(SIZES["ns"])]
        iv = [rnd.randrange(R) for _ in range(SIZES["ninst"])]
        if p % 7 == 3: sc[1] = R + p                    # non-canonical: loads as zero (k_check_scalars reported it)
        if p % 5 == 2: iv[0] = (1 << 256) - 1
        ch = [rnd.randrange(R) for _ in range(SIZES["n_chal"])]
        if p == zero_at: ch[0] = Z_CONST
        envs.append(vr.VmEnv(sc, iv, ch, [rnd.randrange(R)], rnd.randrange(R), 0))
    return envs


def handwritten_program():
    """every opcode; both VM_CONST_OPERAND forms of MUL, ADD and SUB; d == a, d == b; an operand that is the previous result, and one
    that was it two instructions ago; operands 0, 1 and r - 1; POW by 0, 1, 2 and 0xffffffff; SQRN by 0, 1 and 28; an inversion that
    is of zero in the proof whose challenge 0 is consts[4].  Every result goes to a Guard row of its own as it is made (a Guard store
    reads no status), so no intermediate value can hide; the MSM, left and shared rows are stored behind the inversions."""
    C = lambda i: vr.VM_CONST_OPERAND | i
    code, g = [], [0]
    def emit(op, d, a=0, b=0):
        code.append((op, d, a, b))
        code.append((vr.OP_STORE_GUARD, 0, d, g[0])); g[0] += 1
    emit(vr.OP_CONST, 0, 0); emit(vr.OP_CONST, 1, 1); emit(vr.OP_CONST, 2, 2)           # 0, 1, r - 1 (slots 0 and 1: in LDS when two slots are)
    emit(vr.OP_LOAD_SCALAR, 3, 0); emit(vr.OP_LOAD_INST, 4, 1); emit(vr.OP_LOAD_CHAL, 5, 0)
    emit(vr.OP_LOAD_INSTEVAL, 6, 0); emit(vr.OP_LOAD_MULT, 7)
    emit(vr.OP_MUL, 8, 3, 4)
    emit(vr.OP_MUL, 8, 8, 8)          # d == a == b, the previous result
    emit(vr.OP_ADD, 9, 8, 5)          # a: the previous result
    emit(vr.OP_SUB, 10, 3, 9)         # b: the previous result
    emit(vr.OP_MUL, 9, 9, 10)         # d == a; a: the result two instructions ago, b: the previous one
    emit(vr.OP_ADD, 10, 6, 10)        # d == b; b: the result two instructions ago
    emit(vr.OP_MUL, 11, 10, C(3)); emit(vr.OP_MUL, 11, C(5), 11)
    emit(vr.OP_ADD, 11, 11, C(2)); emit(vr.OP_ADD, 11, C(1), 11)
    emit(vr.OP_SUB, 11, 11, C(3)); emit(vr.OP_SUB, 11, C(0), 11)
    emit(vr.OP_MUL, 8, 0, 9); emit(vr.OP_MUL, 8, 1, 9); emit(vr.OP_MUL, 8, 2, 9)        # times 0, 1, r - 1 (an LDS operand and a global one)
    emit(vr.OP_ADD, 8, 2, 1); emit(vr.OP_SUB, 8, 0, 1); emit(vr.OP_ADD, 8, 2, 2)        # r - 1 + 1 = 0, 0 - 1, 2 (r - 1)
    emit(vr.OP_NEG, 8, 0); emit(vr.OP_NEG, 8, 9); emit(vr.OP_NEG, 8, 8)
    for e in (0, 1, 2, 0xffffffff): emit(vr.OP_POW, 8, 9, e)
    emit(vr.OP_POW, 8, 0, 0); emit(vr.OP_POW, 8, 2, 0xffffffff); emit(vr.OP_POW, 8, 8, 2)
    for e in (0, 1, 28): emit(vr.OP_SQRN, 8, 11, e)
    emit(vr.OP_SQRN, 8, 8, 1); emit(vr.OP_SQRN, 1, 2, 28)
    emit(vr.OP_INV, 8, 9); emit(vr.OP_MUL, 8, 8, 9)                                      # x / x = 1
    emit(vr.OP_INV, 0, 2); emit(vr.OP_INV, 8, 8)
    emit(vr.OP_SUB, 10, 5, C(4)); emit(vr.OP_INV, 10, 10)                                # zero in one proof: its status becomes PANIC
    emit(vr.OP_ADD, 10, 10, 7)
    code.append((vr.OP_BARRIER, 0, 0, 0))
    for b, s in enumerate((10, 9, 11, 8, 3, 0)): code.append((vr.OP_STORE_MSM, 0, s, b))
    for b, s in enumerate((7, 10, 6, 1, 4, 2)): code.append((vr.OP_STORE_LEFT, 0, s, b))
    for b, s in enumerate((10, 5, 9, 11)): code.append((vr.OP_STORE_SHARED, 0, s, b))
    while g[0] < SIZES["n_guard"]: code.append((vr.OP_STORE_GUARD, 0, 10, g[0])); g[0] += 1
    assert g[0] == SIZES["n_guard"], g[0]
    return code


def _enc_frvm(code, forms, consts, envs, streams, lds_kb):
    n = len(envs)
    ns, ninst = SIZES["ns"], SIZES["ninst"]
    head = W(n, len(code), N_SLOTS, len(consts), ns, ninst, SIZES["n_chal"], SIZES["n_insteval"], SIZES["np"], SIZES["n_guard"], SIZES["n_shared"], 32 * ns, streams, lds_kb)
    body = b"".join(W(*i) for i in code)
    for K in (2, 3, 4):
        st = forms[K]
        head += W(N_SLOTS, *[len(st[w]) if w < K else 0 for w in range(4)])
        body += b"".join(W(*i) for w in range(K) for i in st[w])
    body += b"".join(vr.le32(c) for c in consts) + W(*[32 * i for i in range(ns)])
    body += b"".join(vr.le32(v) for e in envs for v in e.scalars) + b"".join(vr.le32(v) for e in envs for v in e.inst)
    body += b"".join(vr.le32(e.chal[c]) for c in range(SIZES["n_chal"]) for e in envs)
    body += b"".join(vr.le32(e.insteval[c]) for c in range(SIZES["n_insteval"]) for e in envs)
    body += b"".join(vr.le32(e.mult) for e in envs) + W(*[e.status for e in envs])
    return head + body


VARIANTS = [(streams, kb) for streams in (1, 2, 3, 4) for kb in (1, 5, 156)]      # k_frvm, k_frvm2 with K = 2, 3, 4; 0, 2 and all slots in LDS


def _run_programs(programs, n, tmp_path, seed, zero_at=None, preset=None):
    """every program in all twelve variants on the same n proofs: every variant equals the reference, and so they equal each other"""
    rnd = random.Random(seed)
    jobs, wants = [], []
    for name, code in programs:
        consts, envs = _consts(rnd), _envs(rnd, n, zero_at)
        for p, st in (preset or {}).items():
            if p < n: envs[p].status = st
        forms = {K: vr.vm_split(code, K, N_SLOTS) for K in (2, 3, 4)}
        want = [vr.vm_run(code, consts, e, SIZES["np"], SIZES["n_guard"], SIZES["n_shared"]) for e in envs]
        for streams, kb in VARIANTS:
            jobs.append(_enc_frvm(code, forms, consts, envs, streams, kb))
            wants.append((f"{name}, {streams} stream(s), force_lds_kb={kb}, n={n}", want))
    out = Cursor(_run("frvm", jobs, tmp_path))
    for what, want in wants:
        for ch, cnt in (("msm", SIZES["np"]), ("left", SIZES["np"]), ("guard", SIZES["n_guard"])):
            for p in range(n):
                for b in range(cnt):
                    v = out.num()
                    assert v == want[p][ch][b], f"{what}: proof {p} {ch} row {b} is {v:#x}, not {want[p][ch][b]:#x}"
        for b in range(SIZES["n_shared"]):
            for p in range(n):
                v = out.num()
                assert v == want[p]["shared"][b], f"{what}: proof {p} shared row {b} is {v:#x}, not {want[p]['shared'][b]:#x}"
        for p in range(n):
            st = out.sword()
            assert st == want[p]["status"], f"{what}: proof {p} status {st}, not {want[p]['status']}"
    out.done()
    return [w for _, w in wants]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_frvm_handwritten_program(n, tmp_path):
    zero_at = n // 2
    wants = _run_programs([("the hand-written program", handwritten_program())], n, tmp_path, 4600 + n, zero_at=zero_at,
                          preset={n - 1: vr.ST_OPENING} if n > 1 else None)
    w = wants[0]
    # the program did what it was written for: the inversion of zero in one proof only, whose zeroing stores are zero and whose Guard's is not
    assert [p for p in range(n) if w[p]["status"] == vr.ST_PANIC] == [zero_at]
    assert all(v == 0 for ch in ("msm", "left", "shared") for v in w[zero_at][ch]) and w[zero_at]["guard"][-1] != 0
    if n > 1:   # a status that was set before the program ran zeroes the same stores
        assert w[n - 1]["status"] == vr.ST_OPENING and all(v == 0 for v in w[n - 1]["msm"]) and any(v != 0 for v in w[0]["msm"])


@pytest.mark.parametrize("n", [1, 63, 64, 65, 130])
def test_frvm_random_programs(n, tmp_path):
    rnd = random.Random(4700)
    sizes = dict(SIZES, n_guard=SIZES["n_guard"])
    programs = [(f"random program {i}", vr.vm_random_program(rnd, N_SLOTS, 70, sizes)) for i in range(3)]
    _run_programs(programs, n, tmp_path, 4800 + n)


# ------------------------------------------------------------------ folds
def _rows(out, n):
    return [out.num() for _ in range(n)]


def test_fold_shared(tmp_path):
    rnd = random.Random(4900)
    jobs, meta = [], []
    for gs in (1, 255, 256, 257, 1000):
        for groups in (1, 3):
            for n_shared in (1, 5):
                n, np = gs * groups, 2
                sh = [[rnd.randrange(R) for _ in range(n)] for _ in range(n_shared)]
                jobs.append(W(0, n, np, n_shared, groups, 0) + b"".join(vr.le32(v) for row in sh for v in row))
                meta.append(([gs] * groups, n_shared, n, np, sh))
    # unequal groups, by their offsets: a group below, at and above the 256-lane stride, and a one-proof group between large ones
    for sizes in ([1], [1, 255, 256, 257], [257, 1, 1000]):
        for n_shared in (1, 5):
            n, np = sum(sizes), 2
            off = [sum(sizes[:g]) for g in range(len(sizes) + 1)]
            sh = [[rnd.randrange(R) for _ in range(n)] for _ in range(n_shared)]
            jobs.append(W(0, n, np, n_shared, len(sizes), 1, *off) + b"".join(vr.le32(v) for row in sh for v in row))
            meta.append((sizes, n_shared, n, np, sh))
    out = Cursor(_run("fold", jobs, tmp_path))
    fill = int.from_bytes(FILL32, "little")
    for sizes, n_shared, n, np, sh in meta:
        groups = len(sizes)
        rows = _rows(out, n * np + groups * n_shared)
        what = f"fold_shared sizes={sizes} n_shared={n_shared}"
        assert all(v == fill for v in rows[:n * np]), f"{what}: a row of the proofs' own scalars was written"
        for g in range(groups):
            for j in range(n_shared):
                v, w = rows[n * np + g * n_shared + j], vr.fold(sh, n, j, sum(sizes[:g]), sizes[g])
                assert v == w, f"{what}: group {g} row {j} is {v:#x}, not {w:#x}"
    out.done()


def test_fold_ranges(tmp_path):
    rnd = random.Random(5000)
    fill = int.from_bytes(FILL32, "little")
    def batch(n, n_shared): return [[rnd.randrange(R) for _ in range(n)] for _ in range(n_shared)]
    def enc(batches, ranges, max_shared, out_rows):
        b = W(1, len(batches))
        for sh in batches: b += W(len(sh[0]), len(sh)) + b"".join(vr.le32(v) for row in sh for v in row)
        b += W(len(ranges)) + b"".join(W(*r) for r in ranges) + W(max_shared, out_rows)
        return b
    jobs = []
    # one batch: counts 1, 63, 64, 65 and 200 with first > 0, their output rows interleaved (not in range order), and an empty range
    b0 = batch(300, 3)
    r0 = [(0, 7, 1, 12), (0, 1, 63, 3), (0, 100, 64, 18), (0, 235, 65, 0), (0, 100, 200, 9), (0, 299, 1, 15), (0, 5, 0, 6)]
    jobs.append(([b0], r0, 3, 21))
    # two batches of different keys in one grid: n_shared 2 and 5 under max_shared = 5, every range five rows apart — rows 2..4 of the
    # first batch's ranges stay as they were
    b1, b2 = batch(130, 2), batch(70, 5)
    r1 = [(0, 3, 65, 0), (1, 1, 64, 5), (0, 129, 1, 10), (1, 0, 70, 15), (0, 0, 130, 20)]
    jobs.append(([b1, b2], r1, 5, 25))
    out = Cursor(_run("fold", [enc(*j) for j in jobs], tmp_path))
    for ji, (batches, ranges, max_shared, out_rows) in enumerate(jobs):
        rows, want = _rows(out, out_rows), [fill] * out_rows
        for bi, first, count, o in ranges:
            for j in range(len(batches[bi])): want[o + j] = vr.fold(batches[bi], len(batches[bi][0]), j, first, count)
        for i in range(out_rows):
            assert rows[i] == want[i], f"fold ranges job {ji}: row {i} is {rows[i]:#x}, not {want[i]:#x}" + (" (nothing should have written it)" if want[i] == fill else "")
        if ji == 1: assert [i for i in range(out_rows) if want[i] == fill] == [2, 3, 4, 12, 13, 14, 22, 23, 24]
    out.done()
