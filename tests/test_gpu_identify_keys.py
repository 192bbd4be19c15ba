"""Which proofs made a batch over several VerifyingKeys and instance shapes fail: h2v_verify_batch_keys_identify (the (key, shape)
groups stay resident, and the failing ranges of all groups are searched together, one set of re-check launches per round) and
h2v_batches_recheck (ranges of several finished batches in one set of launches).  Identification must give, proof for proof, what
SingleStrategy gives (h2v_verify_each on the proof's key, the CPU oracle), and leave the accumulation's own result exactly as
h2v_verify_batch_keys gives it.  The bad proofs decode and pass the transcript: only the pairing rejects them."""
import ctypes
import random

import pytest

import circuits
from circuits import R_MOD
from test_gpu_identify import _make_bad

pytestmark = pytest.mark.gpu

CSF, BAD_ARGUMENT = -2, -16


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript, circuit_instances=s.circuit_instances)


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


@pytest.fixture(scope="module")
def two_keys():
    """vector-mul with n_mul 8 and 4 over one params, 256 proofs each, and a context per key"""
    s8, s4 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4)
    assert s8.params == s4.params and s8.vk != s4.vk
    P8, I8 = circuits.prove_vector_mul_batch(s8, 256, seed=61, threads=16)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 256, seed=62, threads=16)
    c8, c4 = _ctx(s8), _ctx(s4)
    yield [s8, s4], [(P8, I8), (P4, I4)], [c8, c4]
    c8.close(); c4.close()
    s8.free(); s4.free()


def _interleaved(pools, n):
    """n proofs, keys in turn (0, 1, 0, 1, ...), each key's pool cycled -> (keys, proofs, instances)"""
    keys, P, I = [], [], []
    for i in range(n):
        k = i % len(pools)
        Pk, Ik = pools[k]
        j = (i // len(pools)) % len(Pk)
        keys.append(k); P.append(Pk[j]); I.append(Ik[j])
    return keys, P, I


def _spoil(keys, P, I, bad, early=()):
    """Copies with pairing-only bad proofs at `bad` (the four kinds in turn, the other proof taken from the same key) and early
    failures at `early` (x >= p, a short proof)"""
    P, I = list(P), list(I)
    for t, i in enumerate(sorted(bad)):
        same = [j for j in range(len(P)) if keys[j] == keys[i] and P[j] != P[i]][:1]
        Pk, Ik = [P[i]] + [P[j] for j in same], [I[i]] + [I[j] for j in same]
        P[i], I[i] = _make_bad(Pk, Ik, 0, t % 4)
    for t, i in enumerate(sorted(early)):
        if t % 2 == 0:
            b = bytearray(P[i]); b[-33] = 0xff; P[i] = bytes(b)
        else:
            P[i] = P[i][:500]
    return P, I


def _expected_statuses(ctxs, keys, P, I):
    """h2v_verify_each on every proof's own key, in call order"""
    out = [None] * len(P)
    for k, c in enumerate(ctxs):
        idx = [i for i in range(len(P)) if keys[i] == k]
        if idx:
            for i, v in zip(idx, c.verify_each([P[i] for i in idx], [I[i] for i in idx])):
                out[i] = v
    return out


def _check(setups, ctxs, keys, P, I, rand, oracle_sample=8):
    """verify_batch_keys_identify against verify_batch_keys, verify_each per key and the oracle's single-proof verdicts"""
    import halo2_verifier_amd as h2v
    ok, st, left, right, checks = h2v.verify_batch_keys_identify(ctxs, keys, P, I, rand)
    assert (ok, left, right) == tuple(h2v.verify_batch_keys(ctxs, keys, P, I, rand)[k] for k in (0, 2, 3))
    assert st == _expected_statuses(ctxs, keys, P, I)
    flagged = [i for i, v in enumerate(st) if v == CSF]
    for i in flagged[:oracle_sample] + flagged[-oracle_sample:]:
        assert circuits.oracle_verify_single(setups[keys[i]], P[i], I[i]) == CSF, i
    if not flagged:
        assert checks == 0
    return ok, st, checks


def test_two_keys_interleaved(two_keys):
    setups, pools, ctxs = two_keys
    n = 1024
    keys, P0, I0 = _interleaved(pools, n)
    rnd = random.Random(5)
    cases = [
        ([], []),
        ([0, 1, n - 2, n - 1], []),                # the first and last proof of each key
        ([500, 501], [77]),                        # adjacent across a key switch, and a proof with x >= p
        (rnd.sample(range(n), 7), [10, 611]),      # scattered, and a short proof
        (list(range(1, n, 2)), []),                # every proof of the second key
    ]
    for t, (bad, early) in enumerate(cases):
        early = [i for i in early if i not in bad]
        P, I = _spoil(keys, P0, I0, bad, early)
        rand = _draws(n, 100 + t)
        ok, st, checks = _check(setups, ctxs, keys, P, I, rand)
        assert ok is (not bad and not early)
        assert [i for i, v in enumerate(st) if v == CSF] == sorted(bad)
        assert all(st[i] not in (0, CSF) for i in early)
        if not bad:
            assert checks == 0
    # the accumulation itself, from the oracle's per-proof Guards (a shorter run of the same interleaving)
    keys, P, I = _interleaved(pools, 64)
    P, I = _spoil(keys, P, I, [9, 40])
    rand = _draws(64, 7)
    exp = circuits.oracle_accumulate([(setups[k], p, i) for k, p, i in zip(keys, P, I)], rand)
    import halo2_verifier_amd as h2v
    ok, st, left, right, checks = h2v.verify_batch_keys_identify(ctxs, keys, P, I, rand)
    assert (ok, left, right) == (exp[0], exp[2], exp[3]) and exp[0] is False
    assert [i for i, v in enumerate(st) if v == CSF] == [9, 40] and checks > 0


def _mixed_lens(s, lens, seed):
    rnd = random.Random(seed)
    P, I = [], []
    for j, m in enumerate(lens):
        a = [rnd.randrange(R_MOD) for _ in range(s.n_mul)]
        b = [rnd.randrange(R_MOD) for _ in range(m)] + [0] * (s.n_mul - m)
        p, inst = circuits.prove_vector_mul_len(s, a, b, m, rng_seed=seed * 100 + j)
        P.append(p); I.append(inst)
    return P, I


def test_instance_shapes(two_keys):
    import halo2_verifier_amd as h2v
    setups, pools, ctxs = two_keys
    s8 = setups[0]
    # one key, several shapes: h2v_verify_batch_shapes' case
    lens = [8, 5, 8, 3, 5, 0, 8, 3] * 4
    P0, I0 = _mixed_lens(s8, lens, 21)
    keys = [0] * len(P0)
    for bad in ([], [0], [3, 5, 30], [1, 2, 3, 4]):
        P, I = _spoil(keys, P0, I0, bad)
        _, st, _ = _check(setups, ctxs, keys, P, I, _draws(len(P), 22))
        assert [i for i, v in enumerate(st) if v == CSF] == bad
    # two keys, the first with two shapes: its first group (shape 8) runs before its second (shape 5) and must stay resident for the
    # search; a bad proof in each group of the first key
    Pa, Ia = _mixed_lens(s8, [8, 5] * 24, 23)
    P4, I4 = pools[1]
    keys, P0, I0 = [], [], []
    for j in range(48):
        keys += [0, 1]; P0 += [Pa[j], P4[j]]; I0 += [Ia[j], I4[j]]
    for bad in ([0], [2], [0, 2, 95], [4, 51]):
        P, I = _spoil(keys, P0, I0, bad)
        _, st, checks = _check(setups, ctxs, keys, P, I, _draws(len(P), 24))
        assert [i for i, v in enumerate(st) if v == CSF] == bad and checks > 0
    # the same proofs as an accumulation
    acc = h2v.AccumulatorStrategy(h2v.ParamsKZG(s8.params, h2v.SerdeFormat.RawBytes), rand=_draws(len(P), 24))
    vks = [h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes) for s in setups]
    for k, p, i in zip(keys, P, I):
        h2v.verify_proof(acc.params, vks[k], acc, i, p)
    assert acc.finalize_identify() is False
    assert [i for i, v in enumerate(acc.statuses) if v == CSF] == [4, 51] and acc.last_range_checks > 0


def test_four_keys_with_their_own_options():
    s8 = circuits.setup_vector_mul(8, 8)
    s9 = circuits.setup_vector_mul(9, 8, s_seed=42)
    ssh = circuits.setup_shuffle(8, s_seed=42).set_options(circuits.GWC, circuits.KECCAK256)
    sw = circuits.setup_wide(8, s_seed=42).set_circuit_instances(2)
    setups = [s8, s9, ssh, sw]
    P8, I8 = circuits.prove_vector_mul_batch(s8, 8, seed=71, threads=8)
    P9, I9 = circuits.prove_vector_mul_batch(s9, 8, seed=72, threads=8)
    Psh, Ish = zip(*[circuits.prove_shuffle(ssh, data_seed=5 + j, rng_seed=90 + j) for j in range(4)])
    Pw, Iw = zip(*[circuits.prove_wide_multi(sw, 2, witness_seed=3 + j, rng_seed=130 + j) for j in range(4)])
    pools = [(P8, I8), (P9, I9), (list(Psh), list(Ish)), (list(Pw), list(Iw))]
    order = [0, 1, 2, 3, 0, 0, 1, 2, 3, 1, 0, 2, 1, 3, 0, 1, 3, 0, 1, 2]
    keys, P0, I0, used = [], [], [], [0, 0, 0, 0]
    for k in order:
        keys.append(k); P0.append(pools[k][0][used[k]]); I0.append(pools[k][1][used[k]]); used[k] += 1
    ctxs = [_ctx(s) for s in setups]
    # one bad proof per key; the shuffle key has no public input: kinds 1 - 3 only
    bad = [4, 6, 7, 13]
    P, I = list(P0), list(I0)
    for t, i in enumerate(bad):
        same = [j for j in range(len(P)) if keys[j] == keys[i] and P[j] != P[i]][:1]
        P[i], I[i] = _make_bad([P[i]] + [P[j] for j in same], [I[i]] + [I[j] for j in same], 0, 1 + t % 3)
    assert sorted({keys[i] for i in bad}) == [0, 1, 2, 3]
    rand = _draws(len(P), 8)
    ok, st, checks = _check(setups, ctxs, keys, P, I, rand)
    assert ok is False and [i for i, v in enumerate(st) if v == CSF] == bad and checks > 0
    exp = circuits.oracle_accumulate([(setups[k], p, i) for k, p, i in zip(keys, P, I)], rand)
    assert exp[0] is False
    for c in ctxs:
        c.close()
    for s in setups:
        s.free()


def _raw_identify(ctxs, keys, P, I, rand_bytes):
    """h2v_verify_batch_keys_identify with every argument as given -> (rc, statuses, ok, checks, left, right)"""
    from halo2_verifier_amd import _lib
    lib = _lib.load_library()
    n = len(P)
    PA = ctypes.c_char_p * max(n, 1)
    ca = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    ka = (ctypes.c_uint32 * max(n, 1))(*keys)
    pl = (ctypes.c_size_t * max(n, 1))(*[len(p) for p in P])
    ia = PA(*[b"".join(v for col in inst for v in col) for inst in I])
    ncols = [len(next(I[i] for i in range(n) if keys[i] == k)) for k in range(len(ctxs))]
    nca = (ctypes.c_size_t * len(ncols))(*ncols)
    cl = [len(col) for inst in I for col in inst]
    cla = (ctypes.c_size_t * max(len(cl), 1))(*cl)
    st = (ctypes.c_int * max(n, 1))(*([5] * n))
    ok, checks = ctypes.c_int(7), ctypes.c_size_t(9)
    left, right = ctypes.create_string_buffer(b"\x11" * 64, 64), ctypes.create_string_buffer(b"\x22" * 64, 64)
    rc = lib.h2v_verify_batch_keys_identify(ca, len(ctxs), ka, n, PA(*P), pl, ia, nca, cla, rand_bytes, st, ctypes.byref(ok), left, right, ctypes.byref(checks))
    return rc, list(st)[:n], ok.value, checks.value, left.raw, right.raw


def test_transcript_error_only_and_zero_draw(two_keys):
    setups, pools, ctxs = two_keys
    keys, P, I = _interleaved(pools, 64)
    # a proof with x >= p contributes nothing: the pairing of the others passes, so there is nothing to search for
    P, I = _spoil(keys, P, I, [], [17])
    rand = _draws(64, 9)
    ok, st, checks = _check(setups, ctxs, keys, P, I, rand)
    assert ok is False and st[17] not in (0, CSF) and st.count(0) == 63 and checks == 0
    # a zero draw: refused before any device work, nothing written
    rand[30] = 0
    rb = b"".join(r.to_bytes(32, "little") for r in rand)
    rc, st, okv, checks, left, right = _raw_identify(ctxs, keys, P, I, rb)
    assert rc == BAD_ARGUMENT
    assert st == [5] * 64 and okv == 7 and checks == 9 and left == b"\x11" * 64 and right == b"\x22" * 64


def test_a_round_wider_than_one_set_of_launches(two_keys):
    setups, pools, ctxs = two_keys
    n = 1024
    keys, P0, I0 = _interleaved(pools, n)
    bad = sorted(random.Random(3).sample(range(n), 600))
    P, I = _spoil(keys, P0, I0, bad)
    ok, st, checks = _check(setups, ctxs, keys, P, I, _draws(n, 10), oracle_sample=4)
    assert ok is False and [i for i, v in enumerate(st) if v == CSF] == bad
    assert checks > 512   # (at least one round took more than MSM_MAX_PROBLEMS / 2 ranges)


def test_sixty_four_groups():
    """one key with 64 instance shapes (inst_len 0 .. 63): the documented maximum of (key, shape) groups in one call"""
    s = circuits.setup_vector_mul(8, 63)
    ctx = _ctx(s)
    lens = list(range(64)) * 2
    P0, I0 = _mixed_lens(s, lens, 31)
    keys = [0] * len(P0)
    bad = [1, 5, 64, 77, 127]   # (a wrong public input needs one: proof 0 has none)
    P, I = _spoil(keys, P0, I0, bad, [40])
    ok, st, checks = _check([s], [ctx], keys, P, I, _draws(len(P), 32))
    assert ok is False and [i for i, v in enumerate(st) if v == CSF] == bad and checks > 0
    ctx.close()
    s.free()


def _staged(ctx, P, I, rand, groups=1):
    import halo2_verifier_amd as h2v
    b = h2v.Batch(ctx, len(P), 64, groups=groups)
    flat, inst = b"".join(P), b"".join(b"".join(col) for i in I for col in i)
    b.upload(flat, len(P[0]), inst, [len(c) for c in I[0]], b"".join(r.to_bytes(32, "little") for r in rand))
    b.launch()
    return b


def test_recheck_batches(two_keys):
    import halo2_verifier_amd as h2v
    setups, pools, ctxs = two_keys
    (P8, I8), (P4, I4) = pools
    s8, s4 = setups
    rnd = random.Random(12)
    # batch A: key 8, 64 proofs; batch B: key 4, 48 proofs; batch C: key 8, two groups of 32.  Every range ends at or after its
    # group's cut, and the draws after the cut are 1: the oracle over the range alone gives the same multipliers
    def draws(n, cut):
        return [rnd.randrange(1, R_MOD) for _ in range(cut)] + [1] * (n - cut)
    keysA, keysB = [0] * 64, [1] * 48
    PA, IA = _spoil(keysA, P8[:64], I8[:64], [42])
    PB, IB = _spoil(keysB, P4[:48], I4[:48], [3])
    PC, IC = _spoil([0] * 64, P8[64:128], I8[64:128], [51])
    rA, rB, rC = draws(64, 40), draws(48, 30), draws(32, 20) + draws(32, 20)
    A, B, C = _staged(ctxs[0], PA, IA, rA), _staged(ctxs[1], PB, IB, rB), _staged(ctxs[0], PC, IC, rC, groups=2)
    fA, fB, fC = A.finish(), B.finish(), C.finish_groups()
    assert fA[0] is False and fB[0] is False and fC[0] == [True, False]
    ranges = [(0, 0, 64), (1, 0, 48), (2, 0, 32), (2, 32, 32), (0, 39, 1), (1, 29, 1), (1, 3, 30), (0, 42, 1), (2, 51, 1), (2, 40, 20),
              (0, 41, 23), (1, 47, 1), (2, 20, 12), (0, 5, 40), (2, 63, 1)]
    batches = [A, B, C]
    data = [(s8, PA, IA, rA), (s4, PB, IB, rB), (s8, PC, IC, rC)]
    oks, lefts, rights = h2v.recheck_batches(batches, ranges)
    for (k, f, c), ok, l, r in zip(ranges, oks, lefts, rights):
        s, P, I, rand = data[k]
        assert (ok, l, r) == tuple(circuits.oracle_verify_batch(s, P[f:f + c], I[f:f + c], rand[f:f + c])[j] for j in (0, 2, 3)), (k, f, c)
    # bit for bit each batch's own re-check of the same ranges
    for k, bt in enumerate(batches):
        mine = [(f, c) for kk, f, c in ranges if kk == k]
        at = [i for i, (kk, _, _) in enumerate(ranges) if kk == k]
        assert bt.recheck(mine) == ([oks[i] for i in at], [lefts[i] for i in at], [rights[i] for i in at])
    # a batch twice in the list
    assert h2v.recheck_batches([A, B, A], [(2, 42, 1), (0, 0, 64), (1, 3, 30)])[0] == [False, False, False]
    # the finished results are unchanged
    assert (A.finish(), B.finish(), C.finish_groups()) == (fA, fB, fC)
    # refusals: a range crossing a group, a batch over other params, a batch not finished
    for bad_ranges in ([(2, 20, 20)], [(0, 60, 5)], [(3, 0, 1)]):
        with pytest.raises(h2v.H2VError) as e:
            h2v.recheck_batches(batches, bad_ranges)
        assert e.value.code == BAD_ARGUMENT
    so = circuits.setup_vector_mul(8, 8, s_seed=7)
    assert so.params != s8.params
    Po, Io = circuits.prove_vector_mul_batch(so, 4, seed=73, threads=4)
    co = _ctx(so)
    O = _staged(co, Po, Io, [1, 2, 3, 4])
    O.finish()
    with pytest.raises(h2v.H2VError) as e:
        h2v.recheck_batches([A, O], [(0, 0, 1), (1, 0, 1)])
    assert e.value.code == BAD_ARGUMENT
    D = _staged(ctxs[0], PA[:8], IA[:8], rA[:8])   # launched, not finished
    with pytest.raises(h2v.H2VError) as e:
        h2v.recheck_batches([A, D], [(0, 0, 1)])
    assert e.value.code == BAD_ARGUMENT
    D.finish()
    for b in (A, B, C, D, O):
        b.close()
    co.close()
    so.free()
