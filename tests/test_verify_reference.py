"""The big-integer references of tests/verify_reference.py against the oracle library, on the inputs tests/test_gpu_verify_units.py
programs: the point decoding against h2o_g1_decompress, the challenges against h2o_blake2b_personal / h2o_keccak256 and
h2o_fr_from_uniform, and the parts the oracle has no entry point for against their definitions written out another way — so the
references the GPU tests compare with are not merely self-consistent.  No GPU."""
import ctypes
import random

import verify_reference as vr

P, R = vr.P, vr.R


def test_the_facts_the_programmed_encodings_rest_on():
    qr = lambda v: pow(v % P, (P - 1) // 2, P) == 1
    assert all(qr(x ** 3 + 3) for x in (1, 2, 3)) and not qr(4 ** 3 + 3) and not qr(10 ** 3 + 3) and not qr(3)
    assert P < (1 << 254) and vr.BETA != 1 and pow(vr.BETA, 3, P) == 1
    w = vr.omega_of(14)
    assert pow(w, 1 << 14, R) == 1 and pow(w, 1 << 13, R) != 1
    assert [vr.fr_canonical(vr.le32(v)) for v in vr.SCALAR_VALUES] == [True, True, False, False, False, True, True]
    assert all(v >> 224 == R >> 224 for v in vr.SCALAR_VALUES[5:])      # the top word alone does not decide these


def test_point_decoding_matches_the_oracle(oracle):
    n_err = n_ok = n_flipped = 0
    for j in vr.decompress_jobs():
        for p in range(j.n):
            for s in range(j.np):
                enc = j.pts[p][s]
                out, ident = ctypes.create_string_buffer(64), ctypes.c_int(0)
                rc = oracle.h2o_g1_decompress(enc, out, ctypes.byref(ident))
                got = vr.g1_decode(enc)
                # the oracle decodes the identity's encoding; reading it from a transcript fails all the same (it cannot be absorbed)
                if rc != 0 or ident.value: assert got is None, (j.names.get((p, s)), enc.hex()); n_err += 1; continue
                assert got is not None, (j.names.get((p, s)), enc.hex())
                assert vr.le32(got[0]) + vr.le32(got[1]) == out.raw, (j.names.get((p, s)), enc.hex())
                n_ok += 1
                # the flipped sign bit gives the other root
                flip = bytearray(enc); flip[31] ^= 0x40
                other = vr.g1_decode(bytes(flip))
                assert other == (got[0], P - got[1]) and (other[1] & 1) != (got[1] & 1); n_flipped += 1
                assert (vr.phi(got)[1] ** 2 - vr.phi(got)[0] ** 3 - 3) % P == 0 and vr.phi(got) != got
    assert n_err > 100 and n_ok > 1000 and n_flipped == n_ok


def test_ranking_of_the_programmed_faults():
    jobs = vr.decompress_jobs()
    for j in jobs[-2:]:
        st = [s for _, s in vr.decompress_expect(j.proofs(), j.inst(), j.point_offsets, j.scalar_offsets, j.n_main, j.ninst)]
        assert st == [vr.ST_INVALID_INSTANCES, vr.ST_TRANSCRIPT, vr.ST_OPENING, 0]
    seen = {s for j in jobs for _, s in vr.decompress_expect(j.proofs(), j.inst(), j.point_offsets, j.scalar_offsets, j.n_main, j.ninst)}
    assert seen == {0, vr.ST_INVALID_INSTANCES, vr.ST_TRANSCRIPT, vr.ST_OPENING}


def test_absorbed_stream_of_a_contract_table():
    """the table model against the transcript written as calls: common_point, common_scalar, squeeze markers"""
    rnd = random.Random(1)
    j = vr.StreamJob(rnd, 2, vr.contract_table(3, 3, 2, 2, "P0SIP", 2), [1])
    for p in range(2):
        pr, yc, iv = j.proofs[p], j.ycanon[p], j.inst[p]
        x0 = pr[0:31] + bytes([pr[31] & 0x3f]); x1 = pr[32:63] + bytes([pr[63] & 0x3f])
        want = b"\x30\x31" + b"\x01" + x0 + yc[0:32] + b"\x00" + b"\x02" + pr[96:128] + b"\x02" + iv[0:32] + b"\x01" + x1 + yc[32:64] + b"\x51\x52"
        assert j.streams()[p] == want
    assert [vr.stream_words(L, False) for L in (1, 120, 121, 127, 128, 129)] == [16, 16, 32, 32, 32, 32]
    assert [vr.stream_words(L, True) for L in (1, 128, 129, 136, 137)] == [17, 17, 34, 34, 34]


def test_challenges_match_the_oracle(oracle):
    for keccak in (False, True):
        for j in vr.transcript_jobs(keccak)[:4]:
            s = j.streams()[j.n // 2]
            got = vr.challenges(s, j.squeeze_at, keccak)
            for q, L in enumerate(j.squeeze_at):
                wide = ctypes.create_string_buffer(64)
                if keccak:
                    lo, hi = ctypes.create_string_buffer(32), ctypes.create_string_buffer(32)
                    oracle.h2o_keccak256(s[:L] + b"\x0a", L + 1, lo); oracle.h2o_keccak256(s[:L] + b"\x0b", L + 1, hi)
                    wide = lo.raw + hi.raw
                else:
                    oracle.h2o_blake2b_personal(b"Halo2-Transcript", s[:L], L, wide); wide = wide.raw
                c = ctypes.create_string_buffer(32)
                oracle.h2o_fr_from_uniform(wide, c)
                assert int.from_bytes(c.raw, "little") == got[q], (keccak, L)


def test_instance_eval_is_the_lagrange_sum():
    """at a small domain against the basis polynomials multiplied out: l_i(x) = prod_{m != i} (x - w^m) / (w^i - w^m)"""
    rnd = random.Random(2)
    k, n = 3, 8
    w = vr.omega_of(k)
    for rot in (0, 1, -1):
        vals, x = [rnd.randrange(R) for _ in range(6)], rnd.randrange(R)
        want = 0
        for j, a in enumerate(vals):
            i, num, den = (j - rot) % n, 1, 1
            for m in range(n):
                if m != i: num = num * (x - pow(w, m, R)) % R; den = den * (pow(w, i, R) - pow(w, m, R)) % R
            want = (want + a * num * pow(den, -1, R)) % R
        assert vr.instance_eval(vals, rot, x, k) == want
        assert vr.instance_eval(vals[:2] + [R + 1] + vals[3:], rot, x, k) == vr.instance_eval(vals[:2] + [0] + vals[3:], rot, x, k)
        assert vr.instance_eval(vals, rot, pow(w, (3 - rot) % n, R), k) is None


def test_program_interpreter_and_its_stream_split():
    """the interpreter on a program worked out by hand, and the split: the K streams, run segment by segment in any order of the
    streams on one slot file, compute what the single stream computes"""
    C = lambda i: vr.VM_CONST_OPERAND | i
    env = vr.VmEnv([5, R + 1], [7], [11], [13], 17)
    code = [(vr.OP_LOAD_SCALAR, 0, 0, 0), (vr.OP_LOAD_SCALAR, 1, 1, 0), (vr.OP_LOAD_CHAL, 2, 0, 0), (vr.OP_MUL, 3, 0, 2), (vr.OP_SUB, 3, 3, C(0)),
            (vr.OP_INV, 4, 1, 0), (vr.OP_POW, 5, 3, 3), (vr.OP_SQRN, 5, 5, 2), (vr.OP_STORE_GUARD, 0, 5, 0), (vr.OP_STORE_MSM, 0, 5, 0), (vr.OP_STORE_SHARED, 0, 3, 0)]
    got = vr.vm_run(code, [3], env, 1, 1, 1)
    assert got == dict(msm=[0], left=[vr.FILL], guard=[pow(52, 12, R)], shared=[0], status=vr.ST_PANIC)    # (a non-canonical scalar loads as zero)
    assert vr.vm_run(code[:5] + code[6:], [3], env, 1, 1, 1)["msm"] == [pow(52, 12, R)]

    import test_gpu_verify_units as t
    rnd = random.Random(3)
    programs = [t.handwritten_program()] + [vr.vm_random_program(rnd, t.N_SLOTS, 70, t.SIZES) for _ in range(6)]
    for code in programs:
        consts, envs = t._consts(rnd), t._envs(rnd, 5, zero_at=2)
        for K in (2, 3, 4):
            streams = vr.vm_split(code, K, t.N_SLOTS)
            assert sorted(i for s in streams for i in s if i[0] != vr.OP_BARRIER) == sorted(i for i in code if i[0] != vr.OP_BARRIER)
            assert len({sum(1 for i in s if i[0] == vr.OP_BARRIER) for s in streams}) == 1 and all(streams)
            segs = [_segments(s) for s in streams]
            for order in (list(range(K)), list(range(K - 1, -1, -1))):
                merged = [i for g in range(len(segs[0])) for w in order for i in segs[w][g]]
                for e in envs:
                    want = vr.vm_run(code, consts, e, t.SIZES["np"], t.SIZES["n_guard"], t.SIZES["n_shared"])
                    assert vr.vm_run(merged, consts, e, t.SIZES["np"], t.SIZES["n_guard"], t.SIZES["n_shared"]) == want


def _segments(stream):
    out = [[]]
    for i in stream:
        if i[0] == vr.OP_BARRIER: out.append([])
        else: out[-1].append(i)
    return out
