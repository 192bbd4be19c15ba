"""The orchestration of distributed.verify_batch_sharded_identify over gloo with two ranks and no GPU: the device side is a stand-in
(tests/fake_shard.py's OracleBatch with an `identify` of its own: the CPU oracle's SingleStrategy per proof).  What is exercised: every
rank identifies its own shard only and only when the batch failed, the existing status gather carries the result to every rank, a zero
among the common draws is refused on every rank before anything is uploaded, and a shard may be empty."""
import os
import random
import socket
import sys

import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close(); return p


def _factory(setup, log):
    import circuits
    import fake_shard

    class IdentifyingBatch(fake_shard.OracleBatch):
        def upload(self, *a):
            log.append("upload")
            super().upload(*a)

        def identify(self, own_records=None):
            log.append(("identify", own_records is not None, len(self.P)))
            st = [circuits.oracle_verify_single(self.s, p, i) for p, i in zip(self.P, self.I)]
            return st, [not any(v == -2 for v in st)], len(self.P)

    return lambda ctx, n, mi, stream, groups: IdentifyingBatch(setup, groups)


def _worker(rank, world, port, total, bad, q):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import circuits
    from halo2_verifier_amd import distributed as h2d
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = circuits.setup_vector_mul(8, 10)
    P, I = circuits.prove_vector_mul_batch(s, total, seed=6, threads=2)
    for i in bad:                                          # a wrong public input: only the pairing rejects the proof
        I[i] = [[circuits.le32(5)] + I[i][0][1:]]
    rnd = random.Random(77)
    rand = [rnd.randrange(1, R_MOD) for _ in range(total)]

    class Ctx:                      # the stand-in never touches it
        device = 0
    log = []
    got = h2d.verify_batch_sharded_identify(Ctx(), P, I, rand, batch_factory=_factory(s, log), device="cpu")
    ref = circuits.oracle_verify_batch(s, P, I, rand)
    single = [circuits.oracle_verify_single(s, p, i) for p, i in zip(P, I)]
    lo, hi = h2d.shard_bounds(total, world, rank)
    calls = [c for c in log if c != "upload"]
    local = h2d.verify_batch_sharded_local_identify(Ctx(), P, I, rand, 3, batch_factory=_factory(s, []), device="cpu")
    # a zero draw: refused on this rank before its upload (and on the other one: neither enters a collective)
    log.clear()
    zero = list(rand); zero[total - 1] = 0
    refused = False
    try:
        h2d.verify_batch_sharded_identify(Ctx(), P, I, zero, batch_factory=_factory(s, log), device="cpu")
    except ValueError:
        refused = True
    q.put((rank, got[:4] == ref[:1] + (single,) + ref[2:], got[4], calls, (hi - lo), local[:4] == got[:4], refused and not log))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("total,bad", [(7, [1, 5]), (6, []), (1, [0]), (5, [4])])
def test_sharded_identify_two_ranks(total, bad):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, 2, port, total, bad, q)) for r in range(2)]
    for p in procs: p.start()
    for p in procs: p.join(300)
    assert all(p.exitcode == 0 for p in procs)
    res = sorted(q.get(timeout=5) for _ in range(2))
    assert [r[0] for r in res] == [0, 1]
    for rank, equal, checks, calls, shard, local_equal, refused in res:
        assert equal and local_equal and refused
        if bad:   # the batch failed: every rank looks at its own shard (an empty one included), with the record it exported
            assert calls == [("identify", True, shard)] and checks == shard
        else:     # the batch passed: nothing runs
            assert calls == [] and checks == 0
