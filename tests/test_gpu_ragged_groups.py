"""Groups of unequal size in one launch (h2v_batch_set_group_sizes): every group must give bit for bit what h2v_verify_batch over its
proofs and its slice of the draws gives — and, for the first, the last and the largest group, what the CPU oracle gives — whatever
the sizes: a few mixed groups, one large group beside single proofs, 64 and 65 groups (either side of the split pairing's limit) and
300 groups.  Also a bad proof's reach, identify / recheck over unequal groups, the GWC + Keccak plan, switching one object between
equal and unequal groups, the refused calls, and upload_launch."""
import random

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 256, seed=4321, threads=16)
    yield s, P, I
    s.free()


@pytest.fixture(scope="module")
def ctx(pool):
    import halo2_verifier_amd as h2v
    s = pool[0]
    c = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    yield c
    c.close()


def _flat(P, I):
    return b"".join(P), b"".join(b"".join(col) for i in I for col in i)


def _rand_bytes(rand):
    return b"".join(r.to_bytes(32, "little") for r in rand)


def _slices(sizes):
    out, at = [], 0
    for sz in sizes:
        out.append(slice(at, at + sz)); at += sz
    return out


def _ragged(ctx, P, I, rand, sizes, keep=False):
    import halo2_verifier_amd as h2v
    b = h2v.Batch(ctx, len(P), 8)
    b.set_group_sizes(sizes)
    flat, inst = _flat(P, I)
    b.upload(flat, 1024, inst, [8], _rand_bytes(rand))
    b.launch()
    out = b.finish_groups()
    if keep:
        return out, b
    b.close()
    return out


def _mixed(n_groups, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, 5) for _ in range(n_groups)]


CASES = {
    "seven": [1, 7, 24, 3, 1, 64, 5],
    "one_large": [200, 1, 1, 1],
    "64_groups": _mixed(64, 64),
    "65_groups": _mixed(65, 65),
    "300_groups": [1 + (g * 7 % 3 == 0) for g in range(300)],
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_unequal_groups_equal_separate_batches(pool, ctx, name):
    s, P, I = pool
    sizes = CASES[name]
    n = sum(sizes)
    Pn, In = [P[i % 256] for i in range(n)], [I[i % 256] for i in range(n)]    # (300 groups: the pool's proofs, cycled)
    rnd = random.Random(len(sizes) * 1000 + n)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    ok, st, left, right = _ragged(ctx, Pn, In, rand, sizes)
    assert st == [0] * n and ok == [True] * len(sizes)
    largest = max(range(len(sizes)), key=lambda g: sizes[g])
    for g, sl in enumerate(_slices(sizes)):
        ref = ctx.verify_batch(Pn[sl], In[sl], rand[sl])
        assert (ok[g], st[sl], left[g], right[g]) == ref, (name, g)
        if g in (0, len(sizes) - 1, largest):
            assert circuits.oracle_verify_batch(s, Pn[sl], In[sl], rand[sl]) == ref, (name, g)


def test_bad_proofs_fail_only_their_groups(pool, ctx):
    s, P, I = pool
    sizes = [1, 7, 24, 3, 1, 64, 5]
    n = sum(sizes)
    sl = _slices(sizes)
    rnd = random.Random(19)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    # group 2: a wrong public input (its pairing fails, no per-proof status); group 5: an undecodable opening point (a per-proof status)
    I2, P2 = list(I[:n]), list(P[:n])
    a = sl[2].start + 11
    I2[a] = [[circuits.le32(5)] + I[a][0][1:]]
    c = sl[5].start + 40
    bad = bytearray(P2[c]); bad[-33] = 0xff; P2[c] = bytes(bad)
    ok, st, left, right = _ragged(ctx, P2, I2, rand, sizes)
    assert ok == [True, True, False, True, True, False, True]
    assert [i for i, v in enumerate(st) if v] == [c]
    for g, x in enumerate(sl):
        ref = ctx.verify_batch(P2[x], I2[x], rand[x])
        assert (ok[g], st[x], left[g], right[g]) == ref
        if g in (2, 5):
            assert circuits.oracle_verify_batch(s, P2[x], I2[x], rand[x]) == ref


def test_identify_and_recheck_over_unequal_groups(pool, ctx):
    import halo2_verifier_amd as h2v
    s, P, I = pool
    sizes = [5, 40, 1, 17, 2]
    n = sum(sizes)
    sl = _slices(sizes)
    rnd = random.Random(23)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    I2 = list(I[:n])
    bad = [sl[1].start + 3, sl[1].start + 39, sl[3].start + 16]       # pairing-only failures in the groups of 40 and of 17
    for i in bad:
        I2[i] = [[circuits.le32(5)] + I[i][0][1:]]
    (ok, st, left, right), b = _ragged(ctx, P[:n], I2, rand, sizes, keep=True)
    assert ok == [True, False, True, False, True] and st == [0] * n
    statuses, own, checks = b.identify()
    assert own == ok and checks > 0
    assert [i for i, v in enumerate(statuses) if v] == bad and all(statuses[i] == h2v.PlonkError.ConstraintSystemFailure for i in bad)
    for g, x in enumerate(sl):
        ref = ctx.verify_batch_identify(P[:n][x], I2[x], rand[x])
        assert (ok[g], statuses[x], left[g], right[g]) == ref
    # a whole group is a range, and so is a piece of one; a range over a boundary is refused, also where equal groups of n / 5 would take it
    oks, lefts, rights = b.recheck([(sl[1].start, 40), (sl[3].start, 16), (sl[0].start, 5), (sl[4].start + 1, 1)])
    assert oks == [False, True, True, True] and lefts[0] == left[1] and rights[0] == right[1] and lefts[2] == left[0]
    for rng in [(sl[0].start + 4, 2), (sl[1].stop - 1, 2), (0, n), (sl[2].start, 2)]:
        with pytest.raises(h2v.H2VError, match="group boundary"):
            b.recheck([rng])
    assert b.finish_groups() == (ok, st, left, right)    # the launch's results are untouched
    b.close()


def test_zero_below_follows_each_groups_own_draws(pool, ctx):
    import halo2_verifier_amd as h2v
    s, P, I = pool
    sizes = [3, 9, 4]
    n = sum(sizes)
    rand = [7 + i for i in range(n)]
    rand[3 + 5] = 0                                      # inside the group of 9: its first five proofs get a zero multiplier
    (ok, st, left, right), b = _ragged(ctx, P[:n], I[:n], rand, sizes, keep=True)
    for g, x in enumerate(_slices(sizes)):
        assert (ok[g], st[x], left[g], right[g]) == ctx.verify_batch(P[:n][x], I[:n][x], rand[x])
    assert b.recheck([(0, 3), (3 + 5, 4), (12, 4)])[0] == [True, True, True]
    with pytest.raises(h2v.H2VError, match="multiplier is zero"):
        b.recheck([(3 + 4, 5)])
    b.close()


def test_unequal_groups_gwc_keccak():
    s = circuits.setup_vector_mul(8, 4).set_options(circuits.GWC, circuits.KECCAK256)
    P, I = circuits.prove_vector_mul_batch(s, 12, seed=5, threads=4)
    import halo2_verifier_amd as h2v
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                      multiopen=s.multiopen, transcript=s.transcript)
    rnd = random.Random(3)
    rand = [rnd.randrange(1, R_MOD) for _ in range(12)]
    sizes = [1, 6, 2, 3]
    b = h2v.Batch(ctx, 12, 4)
    b.set_group_sizes(sizes)
    flat, inst = _flat(P, I)
    b.upload(flat, len(P[0]), inst, [4], _rand_bytes(rand))
    b.launch()
    ok, st, left, right = b.finish_groups()
    b.close()
    assert ok == [True] * 4
    for g, x in enumerate(_slices(sizes)):
        ref = ctx.verify_batch(P[x], I[x], rand[x])
        assert (ok[g], st[x], left[g], right[g]) == ref
        assert circuits.oracle_verify_batch(s, P[x], I[x], rand[x]) == ref
    ctx.close()
    s.free()


def test_one_object_between_unequal_and_equal_groups(pool, ctx):
    import halo2_verifier_amd as h2v
    s, P, I = pool
    n = 24
    flat, inst = _flat(P[:n], I[:n])
    rnd = random.Random(41)
    rands = [[rnd.randrange(1, R_MOD) for _ in range(n)] for _ in range(3)]
    sizes_a, sizes_b = [2, 19, 3], [10, 1, 1, 1, 11]
    b = h2v.Batch(ctx, n, 8)
    b.set_group_sizes(sizes_a)
    b.upload(flat, 1024, inst, [8], _rand_bytes(rands[0])); b.launch()
    assert b.finish_groups() == _ragged(ctx, P[:n], I[:n], rands[0], sizes_a)
    b.set_groups(4)
    b.upload(flat, 1024, inst, [8], _rand_bytes(rands[1])); b.launch()
    fresh = h2v.Batch(ctx, n, 8, groups=4)
    fresh.upload(flat, 1024, inst, [8], _rand_bytes(rands[1])); fresh.launch()
    assert b.finish_groups() == fresh.finish_groups()
    fresh.close()
    b.set_group_sizes(sizes_b)
    b.upload(flat, 1024, inst, [8], _rand_bytes(rands[2])); b.launch()
    assert b.finish_groups() == _ragged(ctx, P[:n], I[:n], rands[2], sizes_b)
    b.close()


def test_refusals(pool, ctx):
    import torch
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd.distributed import ACC_BYTES
    s, P, I = pool
    n = 12
    flat, inst = _flat(P[:n], I[:n])
    b = h2v.Batch(ctx, n, 8)
    lib, c_sizes = b._lib, h2v.verifier._sizes
    # the C side's own checks (the Python mirror refuses these before it calls)
    assert lib.h2v_batch_set_group_sizes(b._h, c_sizes([3, 0, 2]), 3) == -16
    assert lib.h2v_batch_set_group_sizes(b._h, c_sizes([1] * 513), 513) == -16
    assert lib.h2v_batch_set_group_sizes(b._h, c_sizes([6, 7]), 2) == -16       # above max_proofs
    assert lib.h2v_batch_set_group_sizes(b._h, None, 2) == -16
    b.set_group_sizes([5, 7])
    f11, i11 = _flat(P[:11], I[:11])
    with pytest.raises(h2v.H2VError, match="sum of the group sizes"):
        h2v.verifier.check(lib.h2v_batch_upload(b._h, 11, f11, 1024, i11, 1, c_sizes([8]), None, 0))
    with pytest.raises(h2v.H2VError, match="one draw per proof"):
        h2v.verifier.check(lib.h2v_batch_upload(b._h, n, flat, 1024, inst, 1, c_sizes([8]), _rand_bytes([1] * 14), 14))
    with pytest.raises(h2v.H2VError):                    # nothing uploaded: the failed uploads left the batch empty
        b.launch()
    b.upload(flat, 1024, inst, [8], None)                # OS draws
    b.launch(with_pairing=False)
    rec = torch.zeros(2 * ACC_BYTES, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(h2v.H2VError, match="unequal size") as e:
        b.export_accumulators(rec.data_ptr())
    assert e.value.code == -16
    with pytest.raises(h2v.H2VError, match="unequal size") as e:
        b.fold_check_enqueue(rec.data_ptr(), 1)
    assert e.value.code == -16
    with pytest.raises(h2v.H2VError):                    # a grouped batch has no single verdict
        b.finish()
    ok, st, _, _ = b.finish_groups()
    assert ok == [True, True] and st == [0] * n
    b.close()


def test_upload_launch_equals_upload_and_launch(pool, ctx):
    import halo2_verifier_amd as h2v
    s, P, I = pool
    sizes = [1, 7, 24, 3, 1, 64, 5]
    n = sum(sizes)
    rnd = random.Random(57)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    want = _ragged(ctx, P[:n], I[:n], rand, sizes)
    b = h2v.Batch(ctx, n, 8)
    b.set_group_sizes(sizes)
    flat, inst = _flat(P[:n], I[:n])
    b.upload_launch(flat, 1024, inst, [8], _rand_bytes(rand))
    assert b.finish_groups() == want
    b.launch()                                           # a relaunch of the same upload
    assert b.finish_groups() == want
    b.close()


def test_the_launch_limit_of_cut_problems(pool, ctx):
    """The MSM cuts a problem above 16 384 terms into sub-problems and a launch holds 1024 of them.  A group of `big` proofs has a right-channel
    problem just above that size (two sub-problems) beside its left one: with 510 one-proof groups the launch is 3 + 1020 sub-problems, runs
    cut and equals verify_batch; with 511 it would be 1025 and the upload is refused with H2V_ERR_UNSUPPORTED, the batch left empty."""
    import halo2_verifier_amd as h2v
    s, P, I = pool
    big = 16384 // ctx.proof_shape()["n_points"] + 1
    b = h2v.Batch(ctx, big + 511, 8)
    for ones in (511, 510):
        sizes = [big] + [1] * ones
        n = sum(sizes)
        Pn, In = [P[i % 256] for i in range(n)], [I[i % 256] for i in range(n)]
        rnd = random.Random(900 + ones)
        rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
        flat, inst = _flat(Pn, In)
        b.set_group_sizes(sizes)
        if ones == 511:
            with pytest.raises(h2v.H2VError, match="problem limit") as e:
                b.upload(flat, 1024, inst, [8], _rand_bytes(rand))
            assert e.value.code == -19
            with pytest.raises(h2v.H2VError, match="nothing uploaded"):
                b.launch()
            continue
        b.upload(flat, 1024, inst, [8], _rand_bytes(rand))
        b.launch()
        ok, st, left, right = b.finish_groups()
        assert ok == [True] * len(sizes) and st == [0] * n
        sl = _slices(sizes)
        for g in (0, 1, 255, 510):
            assert (ok[g], st[sl[g]], left[g], right[g]) == ctx.verify_batch(Pn[sl[g]], In[sl[g]], rand[sl[g]]), g
        assert circuits.oracle_verify_batch(s, Pn[sl[510]], In[sl[510]], rand[sl[510]]) == (ok[510], st[sl[510]], left[510], right[510])
    b.close()
