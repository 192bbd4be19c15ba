"""Which proofs made a SHARDED batch fail (distributed.verify_batch_sharded_identify / _local_identify, ShardedBatch.identify): every
rank searches its own shard on the record it exported, nothing but the status gather crosses ranks, and the statuses must be, proof
for proof, what SingleStrategy gives — for every world size.  The batch's own result stays verify_batch's.  The bad proofs decode and
pass the transcript: only the pairing rejects them."""
import random

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


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



@pytest.fixture(scope="module")
def case96(pool):
    """96 proofs, bad at both sides of a shard boundary, the first and the last: the reference results, computed once"""
    s, P0, I0, ctx = pool
    n, bad = 96, [0, 31, 32, 95]
    P, I = _spoil(P0[:n], I0[:n], bad)
    rnd = random.Random(61)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    each = ctx.verify_each(P, I)
    assert [i for i in range(n) if each[i] == -2] == bad
    assert [circuits.oracle_verify_single(s, P[i], I[i]) for i in bad] == [-2] * len(bad)
    ref = ctx.verify_batch(P, I, rand)
    assert (ref[0], ref[2], ref[3]) == tuple(circuits.oracle_verify_batch(s, P, I, rand)[k] for k in (0, 2, 3))
    return P, I, rand, each, ref


@pytest.mark.parametrize("world", [1, 2, 3])
def test_local_identify_is_independent_of_the_world_size(pool, case96, world):
    from halo2_verifier_amd import distributed as h2d
    s, _, _, ctx = pool
    P, I, rand, each, ref = case96
    ok, st, left, right, checks = h2d.verify_batch_sharded_local_identify(ctx, P, I, rand, world)
    assert (ok, left, right) == (ref[0], ref[2], ref[3]) and ok is False
    assert st == each
    assert len(checks) == world and all(c > 0 for c in checks)   # (every shard holds a bad proof here, for every world)
    assert h2d.verify_batch_sharded_local(ctx, P, I, rand, world) == ref


def test_a_clean_shard_runs_no_range_check(pool):
    from halo2_verifier_amd import distributed as h2d
    s, P0, I0, ctx = pool
    n, bad = 96, [0, 31, 64, 95]                           # shards of 32: the middle one, [32, 64), is clean
    P, I = _spoil(P0[:n], I0[:n], bad)
    rnd = random.Random(67)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    ok, st, left, right, checks = h2d.verify_batch_sharded_local_identify(ctx, P, I, rand, 3)
    ref = ctx.verify_batch(P, I, rand)
    assert (ok, left, right) == (ref[0], ref[2], ref[3])
    assert st == ctx.verify_each(P, I) == [-2 if i in bad else 0 for i in range(n)]
    assert checks[1] == 0 and checks[0] > 0 and checks[2] > 0


def test_an_empty_shard(pool):
    from halo2_verifier_amd import distributed as h2d
    s, P0, I0, ctx = pool
    P, I = _spoil(P0[:2], I0[:2], [1])
    rand = [5, 7]
    ok, st, left, right, checks = h2d.verify_batch_sharded_local_identify(ctx, P, I, rand, 3)
    ref = ctx.verify_batch(P, I, rand)
    assert (ok, left, right) == (ref[0], ref[2], ref[3]) and ok is False
    assert st == ctx.verify_each(P, I) == [0, -2]
    assert checks == [0, 0, 0]                             # one-proof shards: the shard's own check IS the proof's


def test_a_shard_above_the_direct_threshold(pool):
    from halo2_verifier_amd import distributed as h2d
    s, P0, I0, ctx = pool
    n = 1200                                               # two shards of 600 > H2V_IDENTIFY_DIRECT: a fan-out round, then singles
    P, I = [P0[i % 256] for i in range(n)], [I0[i % 256] for i in range(n)]
    P[911], I[911] = _make_bad(P, I, 911, 2)
    rnd = random.Random(71)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    ok, st, left, right, checks = h2d.verify_batch_sharded_local_identify(ctx, P, I, rand, 2)
    ref = ctx.verify_batch(P, I, rand)
    assert (ok, left, right) == (ref[0], ref[2], ref[3]) and ok is False
    assert st == [-2 if i == 911 else 0 for i in range(n)]
    assert circuits.oracle_verify_single(s, P[911], I[911]) == -2
    assert checks[0] == 0 and 32 < checks[1] <= 32 + 19    # 32 pieces of 18 or 19 proofs, then the failing piece's proofs


def test_a_zero_draw_raises(pool):
    from halo2_verifier_amd import distributed as h2d
    s, P0, I0, ctx = pool
    rand = [3, 0, 5, 7]
    with pytest.raises(ValueError):
        h2d.verify_batch_sharded_local_identify(ctx, P0[:4], I0[:4], rand, 2)
    with pytest.raises(ValueError):
        h2d.verify_batch_sharded_identify(ctx, P0[:4], I0[:4], rand)
    assert h2d.verify_batch_sharded_local(ctx, P0[:4], I0[:4], rand, 2)[0] is True   # (the plain form takes them)


def _rank_main(rank, world, port, q):
    import os
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import circuits as C
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import distributed as h2d
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)     # RCCL refuses two ranks on one device: gloo carries the records
    s = C.setup_vector_mul(8, 8)
    P, I = C.prove_vector_mul_batch(s, 37, seed=99, threads=4)
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes), device=0)
    rnd = random.Random(3)
    rand = [rnd.randrange(1, C.R_MOD) for _ in range(37)]
    good = h2d.verify_batch_sharded_identify(ctx, P, I, rand)
    for k, i in enumerate((2, 18, 19, 36)):                           # both ranks' shards, both sides of the boundary
        P[i], I[i] = _make_bad(P, I, i, k)
    got = h2d.verify_batch_sharded_identify(ctx, P, I, rand)
    ref = (ctx.verify_batch(P, I, rand), ctx.verify_each(P, I)) if rank == 0 else None
    q.put((rank, good, got, ref))
    dist.barrier()
    dist.destroy_process_group()
    ctx.close()


def test_two_real_ranks_on_one_gpu():
    """verify_batch_sharded_identify with two real ranks (processes) on cuda:0, records over gloo: both ranks return the same statuses,
    equal to verify_each, and verify_batch's verdict and accumulators."""
    import socket
    import torch.multiprocessing as mp
    world = 2
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs: p.start()
    res = sorted((q.get(timeout=600) for _ in range(world)), key=lambda t: t[0])
    for p in procs: p.join(120)
    assert all(p.exitcode == 0 for p in procs)
    batch, each = res[0][3]
    assert [i for i in range(37) if each[i] == -2] == [2, 18, 19, 36]
    for rank, good, got, _ in res:
        assert good[0] is True and good[1] == [0] * 37 and good[4] == 0
        assert (got[0], got[2], got[3]) == (batch[0], batch[2], batch[3]) and got[0] is False
        assert got[1] == each
        assert got[4] > 0
