"""A staged batch finished into device memory (h2v_batch_finish_device; Batch.finish_device / finish_into, ShardedBatch.finish_tensors):
the tensors, read after one stream synchronise, hold bit for bit what finish_groups returns for the same launch on the same batch —
clean batches, every kind of rejection at the first and last proof of equal and unequal groups, a launch without a pairing, a fold,
a draw fault, the GWC + Keccak plan — and the counts, indices and summary that tests/results_reference.py derives from those
statuses; before and after the host finish, twice, and after a relaunch; the refusals before any device work; no host wait behind a
busy stream.  Torch tensors are the device memory."""
import ctypes
import random
import time

import pytest

import circuits
import results_reference as rr
from circuits import R_MOD

pytestmark = pytest.mark.gpu

PLEN = 1024
RAGGED = [1, 7, 24, 3, 1]


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 36, seed=9753, threads=16)
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


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


def _batch(ctx, n, groups=1, sizes=None, values=8):
    import halo2_verifier_amd as h2v
    b = h2v.Batch(ctx, n, values)
    if sizes is not None:
        b.set_group_sizes(sizes)
    elif groups != 1:
        b.set_groups(groups)
    return b


def _launched(ctx, P, I, rand, groups=1, sizes=None, pairing=True, plen=PLEN, values=8):
    b = _batch(ctx, len(P), groups, sizes, values)
    flat, inst = _flat(P, I)
    b.upload(flat, plen, inst, [values], _rand_bytes(rand))
    b.launch(with_pairing=pairing)
    return b


def _tensors(n, G, cap=None):
    """the seven outputs, every byte 0xEE (status / verdict words -286331154, which no launch writes)"""
    import torch
    def full(count, dtype): return torch.full((count,), 0xEE if dtype == torch.uint8 else -286331154, dtype=dtype, device="cuda:0")
    return {"status": full(n, torch.int32), "group_ok": full(G, torch.int32), "left_xy": full(64 * G, torch.uint8).reshape(G, 64),
            "right_xy": full(64 * G, torch.uint8).reshape(G, 64), "group_failed": full(G, torch.int32),
            "failed_index": full(n if cap is None else cap, torch.int32), "summary": full(8, torch.int32)}


def _read(t):
    """after ONE synchronise of the device: the tensors as finish_groups' tuple, and the rest"""
    import torch
    torch.cuda.synchronize()
    G = t["group_ok"].numel()
    left, right = bytes(t["left_xy"].cpu().numpy().tobytes()), bytes(t["right_xy"].cpu().numpy().tobytes())
    fin = ([v == 1 for v in t["group_ok"].tolist()], t["status"].tolist(), [left[64 * g:64 * g + 64] for g in range(G)], [right[64 * g:64 * g + 64] for g in range(G)])
    return fin, t["group_failed"].tolist(), [v & 0xffffffff for v in t["failed_index"].tolist()], [v & 0xffffffff for v in t["summary"].tolist()]


def _finish_device(b, cap=None):
    t = _tensors(b.n, b.groups, cap)
    assert set(t["group_ok"].tolist()) == {-286331154}
    b.finish_into(**t)
    return _read(t)


def _check(got, want, groups, sizes, flags, cap=None, fault=rr.NO_FAULT):
    """got: _read's; want: finish_groups' of the same launch — the tuple is equal, and the rest follows from its statuses"""
    fin, failed, index, summary = got
    assert fin == want
    ok, st = want[0], want[1]
    G = len(sizes) if sizes is not None else groups
    assert failed == rr.group_failed(st, groups, sizes)
    idx = rr.failed_index(st, cap)
    assert index[:len(idx)] == idx and all(v == 0xEEEEEEEE for v in index[len(idx):])
    assert summary == [fault, sum(1 for v in st if v), sum(ok), len(st), G, flags, 0, 0]


def _spoiled(P, I, where):
    """four kinds of rejection at the four proofs `where`: a flipped byte of an evaluation and a wrong public input (only the pairing
    sees them), a scalar that is not canonical (status -5), an opening point that is not decodable (status -4)"""
    P, I = list(P), list(I)
    a, b_, c, d = where
    x = bytearray(P[a]); x[700] ^= 1; P[a] = bytes(x)
    P[b_] = P[b_][:-96] + b"\xff" * 32 + P[b_][-64:]
    I[c] = [[circuits.le32(5)] + I[c][0][1:]]
    y = bytearray(P[d]); y[-33] = 0xff; P[d] = bytes(y)
    return P, I


@pytest.mark.parametrize("groups, n", [(1, 24), (4, 32)])
def test_clean_batch(pool, ctx, groups, n):
    s, P, I = pool
    b = _launched(ctx, P[:n], I[:n], _draws(n, n), groups)
    got = _finish_device(b)
    want = b.finish_groups()
    assert want[0] == [True] * groups and want[1] == [0] * n
    _check(got, want, groups, None, rr.FLAG_PAIRING)
    b.close()


def test_each_kind_of_rejection_in_equal_groups(pool, ctx):
    """G = 4: a byte-tampered proof, a non-canonical scalar, a proof that only the pairing rejects, a clean group; finish_device before
    the host finish, after it, twice, and after a relaunch of the same upload"""
    s, P, I = pool
    n = 32
    P2, I2 = _spoiled(P[:n], I[:n], (3, 8, 23, 15))        # groups 0, 1, 2 and 1 again (its last proof)
    b = _launched(ctx, P2, I2, _draws(n, 41), 4)
    before = _finish_device(b, cap=1)
    want = b.finish_groups()
    assert want[0] == [False, False, False, True] and want[1][8] == -5 and want[1][15] == -4 and sum(1 for v in want[1] if v) == 2
    _check(before, want, 4, None, rr.FLAG_PAIRING, cap=1)
    _check(_finish_device(b), want, 4, None, rr.FLAG_PAIRING)
    _check(_finish_device(b, cap=2), want, 4, None, rr.FLAG_PAIRING, cap=2)
    assert b.finish_groups() == want                        # (the host finish is what it was)
    b.launch()
    _check(_finish_device(b, cap=5), want, 4, None, rr.FLAG_PAIRING, cap=5)
    assert b.finish_groups() == want
    b.close()


def test_first_and_last_proofs_of_unequal_groups(pool, ctx):
    """sizes [1, 7, 24, 3, 1]: the same failures at a group's first and last proof"""
    s, P, I = pool
    n = sum(RAGGED)
    P2, I2 = _spoiled(P[:n], I[:n], (0, 1, 7, 31))           # group 0's only proof, group 1's first and last, group 2's last
    b = _launched(ctx, P2, I2, _draws(n, 43), sizes=RAGGED)
    got = _finish_device(b)
    want = b.finish_groups()
    assert want[0] == [False, False, False, True, True] and [i for i, v in enumerate(want[1]) if v] == [1, 31]
    _check(got, want, 1, RAGGED, rr.FLAG_PAIRING)
    P3, I3 = _spoiled(P[:n], I[:n], (32, 34, 35, 8))         # group 3's first and last, group 4's only proof, group 2's first
    flat, inst = _flat(P3, I3)
    b.upload(flat, PLEN, inst, [8], _rand_bytes(_draws(n, 44)))
    b.launch()
    got = _finish_device(b, cap=1)
    want = b.finish_groups()
    assert want[0] == [True, True, False, False, False] and [i for i, v in enumerate(want[1]) if v] == [8, 34]
    _check(got, want, 1, RAGGED, rr.FLAG_PAIRING, cap=1)
    b.close()


def test_launch_without_a_pairing(pool, ctx):
    """no pairing: the verdict words are not the launch's, and a group is accepted on its statuses alone"""
    s, P, I = pool
    n = 16
    P2, I2 = _spoiled(P[:n], I[:n], (0, 5, 9, 10))
    b = _launched(ctx, P[:n], I[:n], _draws(n, 45), 4)
    b.finish_groups()                                      # (a launch with a pairing first: its verdict words stay behind)
    flat, inst = _flat(P2, I2)
    b.upload(flat, PLEN, inst, [8], _rand_bytes(_draws(n, 46)))
    b.launch(with_pairing=False)
    got = _finish_device(b)
    want = b.finish_groups()
    assert want[0] == [True, False, False, True]
    _check(got, want, 4, None, 0)
    _check(_finish_device(b), want, 4, None, 0)
    b.close()


def test_a_fold_rejects_a_group_through_its_record(pool, ctx):
    """launch, export, fold of the batch's own records with group 1's record reporting two failed proofs: the group is rejected by
    fold_failed alone"""
    import torch
    from halo2_verifier_amd.distributed import ACC_BYTES
    s, P, I = pool
    n, G = 16, 2
    b = _launched(ctx, P[:n], I[:n], _draws(n, 47), G, pairing=False)
    rec = torch.zeros(G * ACC_BYTES, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    b.export_accumulators(rec.data_ptr())
    torch.cuda.synchronize()
    rec[ACC_BYTES] = 2                                     # the record's first word: failed proofs
    torch.cuda.synchronize()
    b.fold_check_enqueue(rec.data_ptr(), 1)
    got = _finish_device(b)
    want = b.finish_groups()
    assert want[0] == [True, False] and want[1] == [0] * n
    _check(got, want, G, None, rr.FLAG_PAIRING | rr.FLAG_FOLDED)
    _check(_finish_device(b), want, G, None, rr.FLAG_PAIRING | rr.FLAG_FOLDED)
    b.close()


def test_a_device_draw_of_r(pool, ctx):
    """the summary names the draw, every verdict is 0, and the host finish afterwards still raises and leaves the batch empty"""
    import torch
    import halo2_verifier_amd as h2v
    s, P, I = pool
    n = 16
    rand = _draws(n, 49)
    rand[9], rand[13] = R_MOD, R_MOD + 1
    flat, inst = _flat(P[:n], I[:n])
    proofs = torch.frombuffer(bytearray(flat), dtype=torch.uint8).reshape(n, PLEN).cuda()
    insts = torch.frombuffer(bytearray(inst), dtype=torch.uint8).reshape(n, 256).cuda()
    draws = torch.frombuffer(bytearray(_rand_bytes(rand)), dtype=torch.uint8).reshape(n, 32).cuda()
    b = _batch(ctx, n, 4)
    b.upload_tensors(proofs, insts, [8], draws)
    b.launch()
    fin, failed, index, summary = _finish_device(b)
    assert fin[0] == [False] * 4 and fin[1] == [0] * n and failed == [0] * 4
    assert summary == [9, 0, 0, n, 4, rr.FLAG_PAIRING, 0, 0]
    with pytest.raises(h2v.H2VError, match="draw 9 "):
        b.finish_groups()
    with pytest.raises(h2v.H2VError, match="nothing uploaded"):
        b.launch()
    with pytest.raises(h2v.H2VError, match="nothing launched"):
        b.finish_into(**_tensors(n, 4))
    # a host upload afterwards: no fault word is left over
    good = _draws(n, 50)
    b.upload(flat, PLEN, inst, [8], _rand_bytes(good))
    b.launch()
    got = _finish_device(b)
    want = b.finish_groups()
    assert want[0] == [True] * 4
    _check(got, want, 4, None, rr.FLAG_PAIRING)
    b.close()


def test_gwc_keccak_plan():
    import halo2_verifier_amd as h2v
    s = circuits.setup_vector_mul(8, 4).set_options(circuits.GWC, circuits.KECCAK256)
    P, I = circuits.prove_vector_mul_batch(s, 12, seed=5, threads=4)
    c = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                    multiopen=s.multiopen, transcript=s.transcript)
    sizes = [1, 6, 2, 3]
    I2 = list(I)
    I2[8] = [[circuits.le32(5)] + I[8][0][1:]]
    b = _launched(c, P, I2, _draws(12, 3), sizes=sizes, plen=len(P[0]), values=4)
    got = _finish_device(b)
    want = b.finish_groups()
    assert want[0] == [True, True, False, True]
    _check(got, want, 1, sizes, rr.FLAG_PAIRING)
    b.close(); c.close(); s.free()


def test_sharded_finish_tensors(pool, ctx):
    """ShardedBatch.finish_tensors (a world of one, no exchange): the dict equals finish()"""
    import torch
    from halo2_verifier_amd import distributed as h2d
    s, P, I = pool
    n, G = 16, 2
    P2 = list(P[:n]); P2[11] = P2[11][:-96] + b"\xff" * 32 + P2[11][-64:]
    sb = h2d.ShardedBatch(ctx, n, 8, groups=G, device="cuda:0")
    flat, inst = _flat(P2, I[:n])
    sb.upload(flat, PLEN, inst, [8], _rand_bytes(_draws(n, 51)))
    sb.launch()
    t = sb.finish_tensors()
    assert t["failed_index"].shape == (n,) and t["left_xy"].shape == (G, 64)
    got = _read(t)
    want = sb.finish()
    assert want[0] == [True, False] and want[1][11] == -5
    assert got[0] == want and got[1] == [0, 1] and got[2][0] == 11 and got[2][1:] == [0xffffffff] * (n - 1)
    assert got[3] == [rr.NO_FAULT, 1, 1, n, G, rr.FLAG_PAIRING, 0, 0]
    sb.batch.close()


def test_refusals_come_before_any_device_work(pool, ctx):
    import numpy as np
    import torch
    import halo2_verifier_amd as h2v
    s, P, I = pool
    n, G = 16, 4
    t = _tensors(n, G)
    torch.cuda.synchronize()
    order = ("status", "group_ok", "left_xy", "right_xy", "group_failed", "failed_index", "summary")
    addr = {k: t[k].data_ptr() for k in order}
    b = _batch(ctx, n, G)
    lib = b._lib

    def call(cap=n, **over):
        a = dict(addr, **over)
        return lib.h2v_batch_finish_device(b._h, *[ctypes.c_void_p(a[k]) for k in order[:6]], cap, ctypes.c_void_p(a["summary"]))

    def refused(match, cap=n, **over):
        assert call(cap, **over) == -16
        assert "h2v_batch_finish_device" in h2v._lib.last_error() and match in h2v._lib.last_error(), h2v._lib.last_error()

    refused("nothing launched")                            # an empty batch
    flat, inst = _flat(P[:n], I[:n])
    b.upload(flat, PLEN, inst, [8], _rand_bytes(_draws(n, 53)))
    refused("nothing launched")                            # ... and an uploaded one, which stays uploaded
    b.launch()
    refused("d_status is not 16-byte aligned", status=addr["status"] + 4)
    refused("d_summary is not 16-byte aligned", summary=addr["summary"] + 8)
    host = np.zeros(4 * n + 64, dtype=np.uint8)
    refused("d_status is not device memory", status=(host.ctypes.data + 15) // 16 * 16)
    seg = next(x for x in torch.cuda.memory_snapshot() if x["address"] <= addr["status"] < x["address"] + x["total_size"])
    end = seg["address"] + seg["total_size"]
    refused("d_status: the bytes the call writes end past", status=end - 4 * n + 16)      # 16 bytes short (the alignment's step)
    refused("d_right_xy: the bytes the call writes end past", right_xy=end - 64 * G + 16)
    refused("d_failed_index: the bytes the call writes end past", failed_index=end - 4 * n + 16)
    assert call(3, failed_index=end - 16) == 0             # a cap that fits: 3 words in the allocation's last 16 bytes
    # (torch's allocator rounds sizes up: the allocation ONE byte short is tests/cpp/device_finish_harness.cpp's, from hipMalloc itself)
    refused("failed_cap is 0", cap=0)
    # the Python mirror refuses what it can see before the library is reached
    with pytest.raises(ValueError, match="16-byte aligned"):
        b.finish_device(status_addr=addr["status"] + 4)
    with pytest.raises(ValueError, match="failed_cap"):
        b.finish_device(failed_index_addr=addr["failed_index"])
    with pytest.raises(TypeError, match="int32"):
        b.finish_into(status=t["status"].to(torch.int64))
    with pytest.raises(ValueError, match=f"must hold {n} elements"):
        b.finish_into(status=t["status"][:n - 1])
    with pytest.raises(ValueError, match="must hold 256 elements"):
        b.finish_into(left_xy=t["left_xy"][:3])
    with pytest.raises(ValueError, match="contiguous"):
        b.finish_into(group_ok=torch.zeros(2 * G, dtype=torch.int32, device="cuda:0")[::2])
    with pytest.raises(ValueError, match="context's device"):
        b.finish_into(summary=t["summary"].cpu())
    with pytest.raises(ValueError, match="no output"):
        b.finish_into()
    # the launch is unaffected
    want = b.finish_groups()
    assert want[0] == [True] * G and want[1] == [0] * n
    _check(_finish_device(b), want, G, None, rr.FLAG_PAIRING)
    b.close()


def test_single_outputs(pool, ctx):
    """one output at a time: the others are not needed"""
    import torch
    s, P, I = pool
    n, G = 16, 4
    P2, I2 = _spoiled(P[:n], I[:n], (0, 5, 9, 10))
    b = _launched(ctx, P2, I2, _draws(n, 55), G)
    t = _tensors(n, G)
    for k in t:
        b.finish_into(**{k: t[k]})
    got = _read(t)
    _check(got, b.finish_groups(), G, None, rr.FLAG_PAIRING)
    b.close()


def test_no_host_wait_behind_a_busy_stream(pool, ctx):
    """about a second of spinning is queued on the batch's stream behind a launch: finish_device returns while it still runs"""
    import torch
    s, P, I = pool
    n, G = 16, 4
    b = _launched(ctx, P[:n], I[:n], _draws(n, 57), G)
    t = _tensors(n, G)
    b.finish_into(**t)                                      # the warm call: the scratch has its size
    want = b.finish_groups()
    stream = torch.cuda.ExternalStream(b.stream, device="cuda:0")
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):                        # how long 10^7 of _sleep's cycles take here
        t0.record(); torch.cuda._sleep(10_000_000); t1.record()
    t1.synchronize()
    cycles = int(10_000_000 * 1000.0 / max(t0.elapsed_time(t1), 1e-3))
    b.launch()
    behind = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        behind.record()
    t = _tensors(n, G)
    began = time.perf_counter()
    b.finish_into(**t)
    took = time.perf_counter() - began
    assert not behind.query(), f"finish_into returned after {took:.3f} s, when the stream's earlier work was done"
    got = _read(t)
    _check(got, want, G, None, rr.FLAG_PAIRING)
    assert b.finish_groups() == want
    b.close()
