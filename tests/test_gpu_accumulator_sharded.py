"""The streaming multi-GPU form, halo2_verifier_amd.distributed.ShardedAccumulator: a resident accumulator per rank, closed by ONE
pairing over the merge of the ranks' exported states.  merge_accumulators_local is the same computation on one GPU; two real ranks
(processes on cuda:0, the states and draws over gloo — RCCL refuses two ranks on one device) must agree bit for bit, and a proof that
only the pairing rejects, fed on rank 1, must show in check_ranks() on both.  Expected values come from the CPU oracle: every
rank's own accumulation (batch_reference.expected), merged by oracle_lib.g1_msm over the draws.  At most three processes hold the GPU:
the test's own and the two ranks."""
import random

import pytest

import batch_reference
import circuits
import oracle_lib
from circuits import R_MOD

pytestmark = pytest.mark.gpu
ZERO = bytes(64)


def _rank_items(s, P, I, rank):
    """the proofs rank `rank` streams, in two legs, and their draws"""
    rnd = random.Random(1000 + rank)
    lo = 5 * rank
    legs = [[(s, P[lo + j], I[lo + j]) for j in range(a, b)] for a, b in ((0, 2), (2, 5))]
    return legs, [[rnd.randrange(1, R_MOD) for _ in leg] for leg in legs]


def _expected(s, per_rank, draws):
    """per_rank: [(legs, leg draws)] -> (ok, left, right, bits) of the merge under `draws`, by the oracle"""
    L = oracle_lib.load()
    owns = [batch_reference.expected([it for leg in legs for it in leg], [d for ds in leg_draws for d in ds]) for legs, leg_draws in per_rank]
    left = oracle_lib.g1_msm(L, draws, [o[2] for o in owns])
    right = oracle_lib.g1_msm(L, draws, [o[3] for o in owns])
    bits = [int(circuits.oracle_pairing_check(s, o[2], o[3])) for o in owns]
    ok = circuits.oracle_pairing_check(s, left, right) and not any(v for o in owns for v in o[1])
    return ok, left, right, bits


def _ctx(h2v, s):
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes), device=0)


def _spoil(s, P, I, i):
    """proof i with a wrong public input: status 0, the pairing fails"""
    inst = [[circuits.le32((int.from_bytes(I[i][0][0], "little") + 1) % R_MOD)] + I[i][0][1:]]
    assert circuits.oracle_verify_single(s, P[i], inst) == -2
    return inst


@pytest.mark.parametrize("world", [1, 2, 3])
def test_merge_accumulators_local_equals_the_oracle(world):
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import distributed as h2d
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 15, seed=71, threads=8)
    I = list(I)
    if world == 3:
        I[6] = _spoil(s, P, I, 6)                                   # on rank 1
    ctx = _ctx(h2v, s)
    per_rank = [_rank_items(s, P, I, r) for r in range(world)]
    accs = []
    for legs, leg_draws in per_rank:
        a = h2v.Accumulator(ctx)
        for leg, ds in zip(legs, leg_draws):
            assert a.process(ctx, None, [p for _, p, _ in leg], [i for _, _, i in leg], ds) == [0] * len(leg)
        accs.append(a)
    draws = [random.Random(72 + world).randrange(1, R_MOD) for _ in range(world)]
    got = h2d.merge_accumulators_local(ctx, accs, draws)
    assert got == _expected(s, per_rank, draws)
    assert got[0] is (world != 3) and got[3] == ([1, 0, 1] if world == 3 else [1] * world)
    with pytest.raises(ValueError):
        h2d.merge_accumulators_local(ctx, accs, [0] * world)        # a zero draw
    ok, left, right, bits = h2d.merge_accumulators_local(ctx, accs)  # OS draws
    assert ok is (world != 3) and bits == got[3] and left != ZERO
    for a in accs:
        a.close()
    ctx.close()
    s.free()


def _rank_main(rank, world, port, q):
    import os
    import sys
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import torch.distributed as dist
    import circuits as C
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import distributed as h2d
    import test_gpu_accumulator_sharded as T
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = C.setup_vector_mul(8, 8)
    P, I = C.prove_vector_mul_batch(s, 10, seed=81, threads=4)
    ctx = T._ctx(h2v, s)
    out = [rank]
    for spoiled in (False, True):
        inst = list(I)
        if spoiled:
            inst[7] = T._spoil(s, P, inst, 7)                       # among rank 1's proofs
        legs, leg_draws = T._rank_items(s, P, inst, rank)
        sa = h2d.ShardedAccumulator(ctx)
        for leg, ds in zip(legs, leg_draws):
            assert sa.process(ctx, None, [p for _, p, _ in leg], [i for _, _, i in leg], ds) == [0] * len(leg)
        fixed = sa.finalize([11 + 2 * r for r in range(world)])
        out += [fixed, sa.check_ranks()]
        drawn = sa.finalize()                                        # rank 0 draws and broadcasts; the ranks' accumulators are unchanged
        out += [drawn, sa.last_draws, sa.check_ranks()]
        try:
            sa.finalize([3, 0])
            out.append("no error")
        except ValueError:
            out.append("refused")
        sa.close()
    q.put(tuple(out))
    dist.barrier()
    dist.destroy_process_group()
    ctx.close()


def test_two_real_ranks_on_one_gpu():
    import socket
    import torch.multiprocessing as mp
    world = 2
    sk = socket.socket(); sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]; sk.close()
    mpc = mp.get_context("spawn")
    q = mpc.Queue()
    procs = [mpc.Process(target=_rank_main, args=(r, world, port, q)) for r in range(world)]
    for p in procs: p.start()
    try:
        res = sorted((q.get(timeout=240) for _ in range(world)), key=lambda t: t[0])
        for p in procs: p.join(60)
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert all(p.exitcode == 0 for p in procs)
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 10, seed=81, threads=4)
    L = oracle_lib.load()
    for block, spoiled in ((0, False), (1, True)):
        inst = list(I)
        if spoiled:
            inst[7] = _spoil(s, P, inst, 7)
        per_rank = [_rank_items(s, P, inst, r) for r in range(world)]
        want = _expected(s, per_rank, [11, 13])
        assert want[0] is (not spoiled) and want[3] == ([1, 0] if spoiled else [1, 1])
        for r in res:
            fixed, bits, drawn, draws, bits2, zero = r[1 + 6 * block: 7 + 6 * block]
            assert fixed == want[:3] and bits == want[3] and bits2 == want[3] and zero == "refused"
            assert drawn == res[0][3 + 6 * block] and draws == res[0][4 + 6 * block]     # both ranks: the same draws, the same result
            cs = [int.from_bytes(draws[32 * k:32 * k + 32], "little") for k in range(world)]
            assert all(0 < c < R_MOD for c in cs)
            assert drawn == _expected(s, per_rank, cs)[:3]
    s.free()
