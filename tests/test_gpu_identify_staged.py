"""Which proofs of a finished STAGED batch fail the pairing (h2v_batch_identify, Batch.identify): whatever closed the launch — its own
pairing checks, none (a shard), or a later fold — and for any group count.  The statuses must be, proof for proof, what SingleStrategy
gives (h2v_verify_each, the CPU oracle); group_own_ok must be the oracle's verdict over the group's proofs alone; and the launch's
own results must survive.  The bad proofs decode and pass the transcript: only the pairing rejects them."""
import random

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu

ACC_BYTES = 1312   # include/h2v.h H2V_ACC_RECORD_BYTES


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 256, seed=9173, threads=16)
    ctx = _ctx(s)
    yield s, P, I, ctx
    ctx.close()
    s.free()


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript)


def _flat(P, I):
    return b"".join(P), b"".join(b"".join(col) for i in I for col in i)


def _rand_bytes(rand):
    return b"".join(r.to_bytes(32, "little") for r in rand)


def _neg(pt):
    b = bytearray(pt); b[31] ^= 0x40   # the sign bit of a compressed G1 point: -P
    return bytes(b)


def _make_bad(P, I, i, kind):
    """Proof i made pairing-only bad (decodes, transcript clean) in one of four ways.  -> (proof, instances)"""
    p, inst = bytearray(P[i]), [list(c) for c in I[i]]
    other = P[(i + 1) % len(P)] if P[(i + 1) % len(P)] != P[i] else P[(i + 2) % len(P)]
    if kind == 0:     # a wrong public input
        v = (int.from_bytes(inst[0][0], "little") + 1) % R_MOD
        inst[0][0] = v.to_bytes(32, "little")
    elif kind == 1:   # the sign of h2 flipped
        p[-1] ^= 0x40
    elif kind == 2:   # the first commitment is another proof's
        p[0:32] = other[0:32]
    else:             # ... and its negation
        p[0:32] = _neg(other[0:32])
    return bytes(p), inst


def _spoil(P, I, bad, early=()):
    """Copies of (P, I) with pairing-only bad proofs at `bad` (kinds in turn) and early failures (x >= p) at `early`"""
    P, I = list(P), list(I)
    for k, i in enumerate(sorted(bad)):
        P[i], I[i] = _make_bad(P, I, i, k % 4)
    for i in early:
        b = bytearray(P[i]); b[-33] = 0xff; P[i] = bytes(b)   # top byte of h1: x >= p
    return P, I


def _staged(ctx, P, I, rand, groups=1, with_pairing=True, capacity=None):
    import halo2_verifier_amd as h2v
    b = h2v.Batch(ctx, capacity or len(P), 8, groups=groups)
    flat, inst = _flat(P, I)
    b.upload(flat, len(P[0]), inst, [8], _rand_bytes(rand))
    b.launch(with_pairing=with_pairing)
    return b


def _own_ok(s, P, I, rand, g, gs):
    """the oracle's pairing over group g's proofs alone (proofs with a non-zero status contribute nothing, and do not clear this bit)"""
    lo, hi = g * gs, (g + 1) * gs
    _, _, left, right = circuits.oracle_verify_batch(s, P[lo:hi], I[lo:hi], rand[lo:hi])
    return circuits.oracle_pairing_check(s, left, right)


@pytest.mark.parametrize("bad", [[], [0, 17, 63]])
def test_one_group_after_a_launch_with_and_without_pairing(pool, bad):
    s, P0, I0, ctx = pool
    n = 64
    P, I = _spoil(P0[:n], I0[:n], bad)
    rnd = random.Random(41 + len(bad))
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    each = ctx.verify_each(P, I)
    assert [i for i in range(n) if each[i] == -2] == bad
    for i in bad:
        assert circuits.oracle_verify_single(s, P[i], I[i]) == -2
    own = _own_ok(s, P, I, rand, 0, n)
    assert own == (not bad)
    for with_pairing in (True, False):
        b = _staged(ctx, P, I, rand, with_pairing=with_pairing)
        first = b.finish_groups()
        st, gok, checks = b.identify()
        assert st == each
        assert gok == [own]
        assert (checks == 0) == (not bad)
        assert b.finish_groups() == first
        b.close()


def test_four_groups_bad_proofs_in_two_of_them(pool):
    s, P0, I0, ctx = pool
    G, gs = 4, 16
    n = G * gs
    bad = [gs, 2 * gs - 1, 3 * gs, 4 * gs - 1]          # the first and the last proof of groups 1 and 3
    early = [3 * gs + 5]
    P, I = _spoil(P0[:n], I0[:n], bad, early)
    rnd = random.Random(43)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    each = ctx.verify_each(P, I)
    assert each == [circuits.oracle_verify_single(s, p, i) for p, i in zip(P, I)]
    assert [i for i in range(n) if each[i] == -2] == bad and [i for i in range(n) if each[i] not in (0, -2)] == early
    for with_pairing in (True, False):
        b = _staged(ctx, P, I, rand, groups=G, with_pairing=with_pairing)
        before = b.finish_groups()
        st, gok, checks = b.identify()
        assert gok == [True, False, True, False] == [_own_ok(s, P, I, rand, g, gs) for g in range(G)]
        assert st == each
        assert 0 < checks <= 2 * gs                        # at most the two failing groups' proofs, one by one
        assert b.finish_groups() == before
        b.close()


def test_identify_after_a_fold_needs_the_batchs_own_records(pool):
    import torch
    import halo2_verifier_amd as h2v
    s, P0, I0, ctx = pool
    n = 64
    bad = [5, 40]
    P, I = _spoil(P0[:n], I0[:n], bad)
    rnd = random.Random(47)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    # the unfolded case
    b = _staged(ctx, P, I, rand, with_pairing=False)
    b.finish()
    unfolded = b.identify()
    assert unfolded[0] == ctx.verify_each(P, I) and unfolded[1] == [False]
    # a second batch (good proofs) whose record joins the fold
    other = _staged(ctx, P0[100:132], I0[100:132], rand[:32], with_pairing=False)
    recs = torch.zeros(2 * ACC_BYTES, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    b.export_accumulators(recs.data_ptr())
    other.export_accumulators(recs.data_ptr() + ACC_BYTES)
    other.finish()
    b.fold_check_enqueue(recs.data_ptr(), 2)
    folded = b.finish()
    assert folded[0] is False
    with pytest.raises(h2v.H2VError) as e:
        b.identify()                                       # the batch's own accumulators are gone
    assert e.value.code == -16
    assert b.finish() == folded
    assert b.identify(recs.data_ptr()) == unfolded
    assert b.identify(recs) == unfolded                    # (a tensor is taken by its address)
    assert b.finish() == folded
    # a corrupted header is refused on the host, and nothing runs
    good_header = recs[:16].clone()
    for at, value in ((4, 0), (4, 7), (0, 3)):             # parts = 0, parts = 7, a failure count the statuses do not have
        recs[at] = value
        torch.cuda.synchronize()
        with pytest.raises(h2v.H2VError) as e:
            b.identify(recs.data_ptr())
        assert e.value.code == -16
        recs[:16] = good_header
    torch.cuda.synchronize()
    assert b.identify(recs.data_ptr()) == unfolded
    # a new launch makes the resident accumulators the batch's own again
    b.launch(with_pairing=False)
    b.finish()
    assert b.identify() == unfolded
    b.close(); other.close()


def test_one_bad_proof_in_1024_takes_two_rounds(pool):
    s, P0, I0, ctx = pool
    n = 1024
    P, I = [P0[i % 256] for i in range(n)], [I0[i % 256] for i in range(n)]
    P[777], I[777] = _make_bad(P, I, 777, 1)
    rnd = random.Random(53)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    b = _staged(ctx, P, I, rand, with_pairing=False)
    b.finish()
    st, gok, checks = b.identify()
    assert st == [-2 if i == 777 else 0 for i in range(n)] and gok == [False]
    assert 0 < checks <= 64                                # 32 pieces of 32, then the failing piece's 32 proofs
    assert circuits.oracle_verify_single(s, P[777], I[777]) == -2
    b.close()


def test_zero_draw_and_unfinished_batches_are_refused(pool):
    import halo2_verifier_amd as h2v
    s, P0, I0, ctx = pool
    G, gs = 2, 16
    n = G * gs
    rnd = random.Random(59)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    b = h2v.Batch(ctx, n, 8, groups=G)
    flat, inst = _flat(P0[:n], I0[:n])
    b.upload(flat, len(P0[0]), inst, [8], _rand_bytes(rand))
    with pytest.raises(h2v.H2VError) as e:
        b.identify()                                       # nothing launched
    assert e.value.code == -16
    b.launch()
    with pytest.raises(h2v.H2VError) as e:
        b.identify()                                       # launched, not finished
    assert e.value.code == -16
    with pytest.raises(h2v.H2VError) as e:
        b.recheck([(0, 4)])                                # (the same refusal as h2v_batch_recheck's; the failed call left the batch as it was)
    assert e.value.code == -16
    first = b.finish_groups()
    assert b.identify() == ([0] * n, [True, True], 0)
    rand[gs + 3] = 0                                       # position 3 of group 1: zeroes the multipliers of its proofs 0 .. 2
    b.upload(flat, len(P0[0]), inst, [8], _rand_bytes(rand))
    b.launch()
    again = b.finish_groups()
    assert again[0] == first[0] and again[1] == first[1]
    with pytest.raises(h2v.H2VError) as e:
        b.identify()
    assert e.value.code == -16
    assert b.finish_groups() == again
    b.close()

