"""A staged batch and a sharded batch driven from a 32-byte seed: Batch.upload_tensors(seed=) — the tail expanded by k_expand_draws on
the batch's stream — gives bit for bit what the same draws give when they are uploaded as a tensor or from the host, and what the
oracle computes with them; the group-major tail of a sharded, grouped batch; the sharded entry point; the finish into device
memory."""
import hashlib

import pytest

import circuits

pytestmark = pytest.mark.gpu

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
PLEN = 1024
SEED = bytes((29 * i + 7) % 256 for i in range(32))


def ref_draws(seed, first, n):
    """the definition, in hashlib -> n integers"""
    return [int.from_bytes(hashlib.blake2b(seed + (first + j).to_bytes(8, "little"), digest_size=64, person=b"h2v-draws-v1").digest(), "little") % R_MOD for j in range(n)]


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 50, seed=97531, threads=16)
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


def _tensors(P, I):
    import torch
    flat, inst = _flat(P, I)
    n = len(P)
    return (torch.frombuffer(bytearray(flat), dtype=torch.uint8).reshape(n, PLEN).cuda(),
            torch.frombuffer(bytearray(inst), dtype=torch.uint8).reshape(n, len(inst) // n).cuda())


def _batch(ctx, n, groups=1, sizes=None):
    import halo2_verifier_amd as h2v
    b = h2v.Batch(ctx, n, 8)
    if sizes is not None:
        b.set_group_sizes(sizes)
    elif groups != 1:
        b.set_groups(groups)
    return b


def _run(ctx, P, I, groups, sizes, how, first=0, n_tail=None):
    """one upload, launch and finish -> (group_ok, statuses, left, right)"""
    import halo2_verifier_amd as h2v
    n = len(P)
    nt = n if n_tail is None else n_tail
    b = _batch(ctx, n, groups, sizes)
    flat, inst = _flat(P, I)
    if how == "seed":
        proofs, insts = _tensors(P, I)
        b.upload_tensors(proofs, insts, [8], seed=SEED, first_index=first, n_tail=n_tail)
        kept = b._keep[2]
        assert tuple(kept.shape) == (nt, 32)            # the expanded tail, held until finish
    elif how == "tensor":
        proofs, insts = _tensors(P, I)
        b.upload_tensors(proofs, insts, [8], rand_tail=h2v.expand_tensor(SEED, first, nt, 0))
    elif how == "host":
        b.upload(flat, PLEN, inst, [8], rand_tail=h2v.expand(SEED, first, nt))
    else:
        b.upload(flat, PLEN, inst, [8], seed=SEED, first_index=first, n_tail=n_tail)
    b.launch()
    out = b.finish_groups()
    b.close()
    return out


def _tampered(pool, n, at):
    s, P, I = pool
    P, I = list(P[:n]), list(I[:n])
    I[at] = [[circuits.le32(5)] + I[at][0][1:]]        # a wrong public input: its group's pairing fails
    return s, P, I


@pytest.mark.parametrize("shape", ["3x16", "unequal"])
def test_seeded_upload_equals_uploaded_draws_and_the_oracle(pool, ctx, shape):
    groups, sizes = (3, None) if shape == "3x16" else (1, [1, 30, 17])
    s, P, I = _tampered(pool, 48, 20)                  # inside the second group of either shape
    runs = [_run(ctx, P, I, groups, sizes, how) for how in ("seed", "tensor", "host", "host_seed")]
    assert runs[0] == runs[1] == runs[2] == runs[3]
    ok, st, left, right = runs[0]
    assert ok == [True, False, True]
    draws = ref_draws(SEED, 0, 48)
    bounds = [0, 16, 32, 48] if sizes is None else [0, 1, 31, 48]
    for g in range(3):
        lo, hi = bounds[g], bounds[g + 1]
        want = circuits.oracle_verify_batch(s, P[lo:hi], I[lo:hi], draws[lo:hi])
        assert (ok[g], st[lo:hi], left[g], right[g]) == tuple(want), g


def test_seeded_tail_longer_than_the_upload_and_a_first_index(pool, ctx):
    """equal groups take n_tail >= n draws, n_tail / groups per group, from any first index: the carry into the index's high word"""
    s, P, I = pool
    first = 2**32 - 20
    runs = [_run(ctx, P[:48], I[:48], 3, None, how, first, 60) for how in ("seed", "tensor", "host")]
    assert runs[0] == runs[1] == runs[2] and runs[0][0] == [True] * 3
    draws = ref_draws(SEED, first, 60)
    for g in range(3):     # group g: its 16 proofs with the first 16 of its 20 draws, scaled by the product of the 4 behind them
        import oracle_lib
        L = oracle_lib.load()
        tail = 1
        for d in draws[20 * g + 16:20 * g + 20]:
            tail = tail * d % R_MOD
        _, _, left, right = circuits.oracle_verify_batch(s, P[16 * g:16 * g + 16], I[16 * g:16 * g + 16], draws[20 * g:20 * g + 16])
        assert runs[0][2][g] == oracle_lib.g1_msm(L, [tail], [left]) and runs[0][3][g] == oracle_lib.g1_msm(L, [tail], [right])


def test_both_forms_together_are_refused(pool, ctx):
    import halo2_verifier_amd as h2v
    s, P, I = pool
    b = _batch(ctx, 4)
    proofs, insts = _tensors(P[:4], I[:4])
    with pytest.raises(ValueError, match="not both"):
        b.upload_tensors(proofs, insts, [8], rand_tail=h2v.expand_tensor(SEED, 0, 4, 0), seed=SEED)
    with pytest.raises(ValueError, match="n_tail"):
        b.upload_tensors(proofs, insts, [8], seed=SEED, n_tail=3)
    b.upload_tensors(proofs, insts, [8], seed=SEED)    # the batch still works
    b.upload_tensors(proofs, insts, [8], seed=SEED)    # ... and a second upload before any finish frees no tail the stream may still read
    assert 1 <= len(b._tails) <= 2 and b._tails[-1][1] is b._keep[2]
    b.launch()
    assert b.finish_groups()[0] == [True] and b._tails == []
    b.close()


def test_sharded_entry_point_from_a_seed(pool, ctx):
    from halo2_verifier_amd import distributed as h2d
    s, P, I = _tampered(pool, 50, 33)
    draws = ref_draws(SEED, 0, 50)
    for Pn, In, verdict in ((pool[1], pool[2], True), (P, I, False)):
        ref = ctx.verify_batch(Pn, In, draws)
        got = h2d.verify_batch_sharded_local(ctx, Pn, In, seed=SEED, world=3)
        assert got == ref and got[0] is verdict
    got = h2d.verify_batch_sharded_local_identify(ctx, P, I, seed=SEED, world=3)
    assert got[0] is False and [i for i, v in enumerate(got[1]) if v] == [33]
    with pytest.raises(ValueError, match="not both"):
        h2d.verify_batch_sharded_local(ctx, P, I, draws, world=3, seed=SEED)


def test_grouped_shards_take_the_group_major_tail(pool, ctx):
    """two independent batches of 25 proofs in one launch, cut into two shards run one after the other: every shard expands, per
    group, the indices from its first proof to the end of the group's batch"""
    import torch
    from halo2_verifier_amd import distributed as h2d
    s, P, I = pool
    total, world, G = 25, 2, 2
    shards = []
    for r in range(world):
        lo, hi = h2d.shard_bounds(total, world, r)
        Ps = [P[g * total + i] for g in range(G) for i in range(lo, hi)]
        Is = [I[g * total + i] for g in range(G) for i in range(lo, hi)]
        sb = h2d.ShardedBatch(ctx, len(Ps), 8, groups=G, world_size=world)
        proofs, insts = _tensors(Ps, Is)
        sb.upload_tensors(proofs, insts, [8], seed=SEED, lo=lo, total=total)
        tail = sb.batch._keep[2]
        assert len(sb.batch._tails) == 1 and sb.batch._tails[0][1] is tail      # the batch holds the tail no caller holds
        torch.cuda.synchronize()                        # (written on the batch's stream, which nothing else waits for)
        assert bytes(tail.cpu().numpy().tobytes()) == h2d.seeded_tail(SEED, lo, total, G)
        sb.launch_shard()
        assert sb.finish()[1] == [0] * len(Ps) and sb.batch._tails == []
        shards.append(sb)
    gathered = torch.cat([sb.records for sb in shards])
    torch.cuda.synchronize()
    shards[0].fold(gathered, world)
    ok, _, left, right = shards[0].finish()
    for g in range(G):
        want = ctx.verify_batch(P[g * total:(g + 1) * total], I[g * total:(g + 1) * total], ref_draws(SEED, g * total, total))
        assert (bool(ok[g]), left[g], right[g]) == (want[0], want[2], want[3]) and want[0] is True
    for sb in shards:
        sb.close()
    with pytest.raises(ValueError, match="lo and total"):
        h2d.ShardedBatch.upload_tensors(shards[0], None, None, [8], seed=SEED)


def test_a_loop_that_never_waits_in_finish_holds_a_bounded_set_of_tails(pool, ctx):
    """upload(seed) / launch / finish_into, again and again on one long-lived batch, with no host finish: a tail is held until the
    batch's stream has passed its upload and is let go at the next upload or finish_into that finds its event complete, so the
    held set is the launches in flight.  The consumer here looks at the results every 8 launches (a synchronise of its stream,
    which finish_into ordered behind the batch's): never more than 8 tails are held, and torch's memory does not grow."""
    import torch
    import halo2_verifier_amd as h2v
    s, P, I = pool
    b = _batch(ctx, 16, 4)
    proofs, insts = _tensors(P[:16], I[:16])
    group_ok = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    summary = torch.zeros(h2v.Batch.SUMMARY_WORDS, dtype=torch.int32, device="cuda:0")
    held, allocated = [], []
    for it in range(48):
        b.upload_tensors(proofs, insts, [8], seed=SEED, first_index=1000 * it, n_tail=64)
        b.launch()
        b.finish_into(group_ok=group_ok, summary=summary)
        held.append(len(b._tails))
        if it % 8 == 7:
            torch.cuda.current_stream().synchronize()
            assert group_ok.tolist() == [1] * 4 and summary.tolist()[0] & 0xffffffff == 0xffffffff
            allocated.append(torch.cuda.memory_allocated())
    assert max(held) <= 8 and all(held[it] <= 1 for it in range(8, 48, 8)), held       # right after a look at the results: the new tail alone
    assert max(allocated) - min(allocated) <= 8 * 64 * 32, allocated
    b._drop_done_tails()
    assert b._tails == []
    assert b.finish_groups()[0] == [True] * 4          # a host finish may still follow
    b.close()


def test_finish_into_after_a_seeded_upload(pool, ctx):
    import torch
    import halo2_verifier_amd as h2v
    s, P, I = pool
    b = _batch(ctx, 16, 4)
    proofs, insts = _tensors(P[:16], I[:16])
    b.upload_tensors(proofs, insts, [8], seed=SEED)
    b.launch()
    summary = torch.zeros(h2v.Batch.SUMMARY_WORDS, dtype=torch.int32, device="cuda:0")
    group_ok = torch.zeros(4, dtype=torch.int32, device="cuda:0")
    b.finish_into(group_ok=group_ok, summary=summary)
    torch.cuda.synchronize()
    assert summary.tolist()[0] & 0xffffffff == 0xffffffff      # no draw fault: every expanded draw is canonical
    assert group_ok.tolist() == [1] * 4
    b.close()
