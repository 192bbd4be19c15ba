"""A sharded batch driven from a 32-byte seed, two ranks over gloo with the stand-in batch of tests/fake_shard.py (no GPU here):
the seed is the only thing broadcast, every rank expands its own tail, and the result is the one of the same draws given
explicitly.  The device side of the same path is tests/test_gpu_draws_batch.py."""
import hashlib
import os
import socket
import sys

import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
TOTAL = 7
SEED = bytes((11 * i + 5) % 256 for i in range(32))


def ref_rows(seed, n):
    return [(int.from_bytes(hashlib.blake2b(seed + i.to_bytes(8, "little"), digest_size=64, person=b"h2v-draws-v1").digest(), "little") % R_MOD).to_bytes(32, "little")
            for i in range(n)]


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import circuits
    import fake_shard
    from halo2_verifier_amd import distributed as h2d, draws
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = circuits.setup_vector_mul(8, 10)
    P, I = circuits.prove_vector_mul_batch(s, TOTAL, seed=6, threads=2)
    factory = fake_shard.make_factory(s)

    class Ctx:                      # the stand-in never touches it
        device = 0

    # every broadcast the product makes, by the bytes it carries
    sent = []
    real_broadcast = dist.broadcast

    def counting_broadcast(tensor, *a, **k):
        sent.append(tensor.numel() * tensor.element_size())
        return real_broadcast(tensor, *a, **k)
    dist.broadcast = counting_broadcast
    try:
        # a given seed: no broadcast at all, and the result of the same draws given as rows
        got = h2d.verify_batch_sharded(Ctx(), P, I, seed=SEED, batch_factory=factory, device="cpu")
        given_broadcasts = list(sent)
        rows = [draws.expand(SEED, 0, TOTAL)[32 * i:32 * i + 32] for i in range(TOTAL)]
        local = h2d.verify_batch_sharded_local(Ctx(), P, I, rows, world=2, batch_factory=factory, device="cpu")
        local_seeded = h2d.verify_batch_sharded_local(Ctx(), P, I, seed=SEED, world=3, batch_factory=factory, device="cpu")
        oracle = circuits.oracle_verify_batch(s, P, I, [int.from_bytes(r, "little") for r in ref_rows(SEED, TOTAL)])
        # seed=True: rank 0 draws, one 32-byte broadcast
        del sent[:]
        drawn = h2d.verify_batch_sharded(Ctx(), P, I, seed=True, batch_factory=factory, device="cpu")
        drawn_broadcasts = list(sent)
        # the draws it used are the seed's, so a second seed gives other accumulators: compare across ranks instead
        seed2 = h2d.common_seed()
        del sent[:]
        # the unseeded path still broadcasts n x 32 bytes (what the seed saves)
        h2d.verify_batch_sharded(Ctx(), P, I, batch_factory=factory, device="cpu")
        plain_broadcasts = list(sent)
        # both forms together are refused on every rank before any collective
        try:
            h2d.verify_batch_sharded(Ctx(), P, I, rows, seed=SEED, batch_factory=factory, device="cpu")
            both = "accepted"
        except ValueError as e:
            both = str(e)
    finally:
        dist.broadcast = real_broadcast
    q.put({"rank": rank, "rows_are_the_definition": rows == ref_rows(SEED, TOTAL), "got": got, "local": local, "local_seeded": local_seeded, "oracle": oracle,
           "given_broadcasts": given_broadcasts, "drawn": drawn, "drawn_broadcasts": drawn_broadcasts, "seed2": seed2, "plain_broadcasts": plain_broadcasts,
           "both": both})
    dist.barrier()
    dist.destroy_process_group()


def test_sharded_batch_from_a_seed_two_ranks():
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs: p.start()
    res = sorted((q.get(timeout=300) for _ in range(2)), key=lambda r: r["rank"])
    for p in procs: p.join(60)
    assert all(p.exitcode == 0 for p in procs)
    a, b = res
    for r in res:
        assert r["rows_are_the_definition"]
        # seed = s: equal to the local form over expand(s, 0, n) as rows, to the seeded local form, and to the oracle with those draws
        assert r["got"] == r["local"] == r["local_seeded"] == r["oracle"] and r["got"][0] is True and r["got"][1] == [0] * TOTAL
        assert r["given_broadcasts"] == []                 # a given seed crosses no collective
        assert r["drawn_broadcasts"] == [32]               # seed=True: the only broadcast made is the seed's 32 bytes
        assert r["plain_broadcasts"] == [32 * TOTAL]       # (the path without a seed: n x 32)
        assert r["both"].startswith("give the draws")
        assert r["drawn"][0] is True and r["drawn"][1] == [0] * TOTAL
    assert a["got"] == b["got"]
    assert a["drawn"] == b["drawn"]                        # seed=True returns the same on both ranks: one seed, one stream of draws
    assert a["drawn"][2:] != a["got"][2:]                  # ... and it is a fresh seed, not the given one
    assert a["seed2"] == b["seed2"] and len(a["seed2"]) == 32 and a["seed2"] != SEED
