"""A staged batch uploaded from device memory (h2v_batch_upload_device; Batch.upload_device / upload_tensors): bit for bit the
(group_ok, statuses, left, right) of Batch.upload of the same bytes, for one group, equal and unequal groups, 65 groups, a padded
row stride, OS draws, a shard, a tampered proof and the GWC + Keccak plan; the same recheck ranges with zero draws; the same
Accumulator.process_batch; the refusals before any device work; the draw fault that arrives with finish(); and no host wait behind
a busy stream.  Torch tensors are the device memory."""
import ctypes
import random
import time

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu

PLEN = 1024


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 64, seed=8642, threads=16)
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


def _cycled(P, I, n):
    return [P[i % len(P)] for i in range(n)], [I[i % len(I)] for i in range(n)]


def _tensors(P, I, rand, stride=None, plen=PLEN):
    """-> (proofs [n, plen] with row stride `stride`, the padding poisoned; instances [n, values * 32]; draws [n_tail, 32] or None)"""
    import torch
    n, stride = len(P), stride or plen
    flat, inst = _flat(P, I)
    rows = torch.full((n, stride), 0xAB, dtype=torch.uint8)
    rows[:, :plen] = torch.frombuffer(bytearray(flat), dtype=torch.uint8).reshape(n, plen)
    proofs = rows.cuda()[:, :plen]
    insts = torch.frombuffer(bytearray(inst), dtype=torch.uint8).reshape(n, len(inst) // n).cuda()
    draws = torch.frombuffer(bytearray(_rand_bytes(rand)), dtype=torch.uint8).reshape(len(rand), 32).cuda() if rand is not None else None
    return proofs, insts, draws


def _batch(ctx, n, groups=1, sizes=None, values=8):
    import halo2_verifier_amd as h2v
    b = h2v.Batch(ctx, n, values)
    if sizes is not None:
        b.set_group_sizes(sizes)
    elif groups != 1:
        b.set_groups(groups)
    return b


def _host(ctx, P, I, rand, groups=1, sizes=None, keep=False, pairing=True):
    b = _batch(ctx, len(P), groups, sizes)
    flat, inst = _flat(P, I)
    b.upload(flat, PLEN, inst, [8], _rand_bytes(rand) if rand is not None else None)
    b.launch(with_pairing=pairing)
    out = b.finish_groups()
    if keep:
        return out, b
    b.close()
    return out


def _device(ctx, P, I, rand, groups=1, sizes=None, keep=False, pairing=True, stride=None):
    b = _batch(ctx, len(P), groups, sizes)
    proofs, insts, draws = _tensors(P, I, rand, stride)
    b.upload_tensors(proofs, insts, [8], draws)
    b.launch(with_pairing=pairing)
    out = b.finish_groups()
    assert b._keep is None      # (the tensors were held until here)
    if keep:
        return out, b
    b.close()
    return out


CASES = {
    "one_proof": (1, 1, None),
    "seven_proofs": (7, 1, None),
    "4x4": (16, 4, None),
    "unequal": (35, 1, [1, 7, 24, 3]),
    "65_groups": (97, 1, [1 + g % 2 for g in range(65)]),
}


@pytest.mark.parametrize("name", list(CASES))
def test_device_upload_equals_host_upload(pool, ctx, name):
    s, P64, I64 = pool
    n, groups, sizes = CASES[name]
    P, I = _cycled(P64, I64, n)
    rand = _draws(n, 100 + n)
    want = _host(ctx, P, I, rand, groups, sizes)
    assert want[0] == [True] * (len(sizes) if sizes else groups) and want[1] == [0] * n
    assert _device(ctx, P, I, rand, groups, sizes) == want


def test_padded_stride_with_poisoned_padding(pool, ctx):
    s, P, I = pool
    rand = _draws(16, 7)
    assert _device(ctx, P[:16], I[:16], rand, 4, stride=PLEN + 64) == _host(ctx, P[:16], I[:16], rand, 4)


def test_os_draws(pool, ctx):
    """rand_tail None: the draws are the library's own, so only the verdicts compare"""
    s, P, I = pool
    ok, st, left, right = _device(ctx, P[:12], I[:12], None, 4)
    assert ok == [True] * 4 and st == [0] * 12 and all(len(p) == 64 and any(p) for p in left + right)


def test_shard_exports_the_same_record(pool, ctx):
    """proofs [0, 8) of a batch of 16, the tail of all 16 draws, no pairing: the exported record and the finished channels"""
    import numpy as np
    import torch
    import msm_reference as ref
    from halo2_verifier_amd.distributed import ACC_BYTES
    s, P, I = pool
    rand = _draws(16, 9)
    recs = []
    for device in (False, True):
        b = _batch(ctx, 8)
        if device:
            proofs, insts, _ = _tensors(P[:8], I[:8], None)
            b.upload_tensors(proofs, insts, [8], _tensors(P[:16], I[:16], rand)[2])
        else:
            flat, inst = _flat(P[:8], I[:8])
            b.upload(flat, PLEN, inst, [8], _rand_bytes(rand))
        rec = torch.zeros(ACC_BYTES, dtype=torch.uint8, device="cuda:0")
        torch.cuda.synchronize()
        b.launch(with_pairing=False)
        b.export_accumulators(rec.data_ptr())
        fin = b.finish()          # (the batch's stream is idle: the record is written)
        words = np.frombuffer(bytes(rec.cpu().numpy().tobytes()), dtype="<u4").tolist()
        # [failed, parts, shift, 0], then 2 x 6 Jacobian pieces of 27 words: the points they stand for (a launch's Jacobian coordinates are
        # one of many forms of the same point, and which one depends on the order its waves ran in)
        recs.append((fin, words[:4], [ref.jac_point(words[4 + 27 * k:31 + 27 * k]) for k in range(12)]))
        b.close()
    assert recs[0][1][1] > 1 and any(p is not None for p in recs[0][2])
    assert recs[0] == recs[1]


def test_tampered_proof_and_identify(pool, ctx):
    s, P, I = pool
    sizes = [1, 7, 24, 3]
    n = sum(sizes)
    rand = _draws(n, 11)
    I2, P2 = list(I[:n]), list(P[:n])
    I2[1 + 4] = [[circuits.le32(5)] + I[5][0][1:]]                    # a wrong public input: the pairing of group 1 fails
    bad = bytearray(P2[8 + 20]); bad[-33] = 0xff; P2[8 + 20] = bytes(bad)   # an undecodable opening point: a per-proof status in group 2
    want, hb = _host(ctx, P2, I2, rand, sizes=sizes, keep=True)
    got, db = _device(ctx, P2, I2, rand, sizes=sizes, keep=True)
    assert want[0] == [True, False, False, True] and got == want
    assert db.identify() == hb.identify()
    hb.close(); db.close()


def test_gwc_keccak_plan():
    import halo2_verifier_amd as h2v
    s = circuits.setup_vector_mul(8, 4).set_options(circuits.GWC, circuits.KECCAK256)
    P, I = circuits.prove_vector_mul_batch(s, 12, seed=5, threads=4)
    c = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                    multiopen=s.multiopen, transcript=s.transcript)
    rand, sizes, plen = _draws(12, 3), [1, 6, 2, 3], len(P[0])
    flat, inst = _flat(P, I)
    hb, db = _batch(c, 12, sizes=sizes, values=4), _batch(c, 12, sizes=sizes, values=4)
    hb.upload(flat, plen, inst, [4], _rand_bytes(rand)); hb.launch()
    proofs, insts, draws = _tensors(P, I, rand, plen + 16, plen)
    db.upload_tensors(proofs, insts, [4], draws); db.launch()
    want = hb.finish_groups()
    assert want[0] == [True] * 4 and db.finish_groups() == want
    hb.close(); db.close(); c.close(); s.free()


@pytest.mark.parametrize("shape", ["equal", "unequal"])
def test_recheck_with_zero_draws(pool, ctx, shape):
    """zero_below comes from the device: recheck refuses and accepts the same ranges as after a host upload"""
    import halo2_verifier_amd as h2v
    s, P, I = pool
    groups, sizes = (2, None) if shape == "equal" else (1, [3, 9, 4])
    rand = [7 + i for i in range(16)]
    rand[3 + 5] = 0        # equal: group 1's first draw — zeroes nobody; unequal: inside the group of 9 — its first five proofs
    rand[1] = 0            # the second draw of group 0: its first proof
    want, hb = _host(ctx, P[:16], I[:16], rand, groups, sizes, keep=True)
    got, db = _device(ctx, P[:16], I[:16], rand, groups, sizes, keep=True)
    assert got == want
    ranges = [(0, 1), (1, 2), (0, 3), (3, 5), (7, 1), (8, 4), (8, 1), (12, 4)]
    for rng in ranges:
        res = []
        for b in (hb, db):
            try:
                res.append(b.recheck([rng]))
            except h2v.H2VError as e:
                res.append((e.code, "multiplier is zero" in str(e), "group boundary" in str(e)))
        assert res[0] == res[1], rng
    with pytest.raises(h2v.H2VError, match="multiplier is zero"):
        db.recheck([(0, 1)])
    assert db.recheck([(1, 2)])[0] == [True]
    with pytest.raises(h2v.H2VError, match="zero multiplier"):
        db.identify()
    hb.close(); db.close()


def test_accumulator_process_batch(pool, ctx):
    import halo2_verifier_amd as h2v
    s, P, I = pool
    sizes = [1, 7, 2, 14]
    rand = _draws(24, 13)
    (want, hb), (got, db) = _host(ctx, P[:24], I[:24], rand, sizes=sizes, keep=True), _device(ctx, P[:24], I[:24], rand, sizes=sizes, keep=True)
    assert got == want
    fed, ref = h2v.Accumulator(ctx, journal=5), h2v.Accumulator(ctx, journal=5)
    assert fed.process_batch(db) == ref.process_batch(hb) == (24, 0)
    assert fed.read() == ref.read() and fed.check_legs() == ref.check_legs()
    assert fed.finalize() == ref.finalize()
    fed.close(); ref.close(); hb.close(); db.close()


def test_refusals_come_before_any_device_work(pool, ctx):
    import numpy as np
    import torch
    import halo2_verifier_amd as h2v
    s, P, I = pool
    rand = _draws(8, 17)
    want = _host(ctx, P[:8], I[:8], rand)
    proofs, insts, draws = _tensors(P[:8], I[:8], rand, PLEN + 64)
    torch.cuda.synchronize()
    b = _batch(ctx, 8)
    lib, sz = b._lib, h2v.verifier._sizes
    pa, ia, ra = proofs.data_ptr(), insts.data_ptr(), draws.data_ptr()

    def call(n, p, stride, i, cols, r, nt):
        return lib.h2v_batch_upload_device(b._h, n, ctypes.c_void_p(p), stride, ctypes.c_void_p(i), len(cols), sz(cols), ctypes.c_void_p(r), nt)

    def refused(match, *args):
        assert call(*args) == -16
        assert match in h2v._lib.last_error(), h2v._lib.last_error()
        with pytest.raises(h2v.H2VError, match="nothing uploaded"):
            b.launch()

    refused("16-byte aligned", 7, pa + 8, PLEN + 64, ia, [8], ra, 7)                       # a misaligned pointer
    refused("16-byte aligned", 7, pa, PLEN + 64, ia, [8], ra + 4, 7)
    refused("proof_stride", 8, pa, PLEN - 16, ia, [8], ra, 8)                              # a stride below proof_len
    refused("proof_stride", 8, pa, PLEN + 8, ia, [8], ra, 8)                               # ... and one that is no multiple of 16
    host = np.zeros(8 * PLEN + 64, dtype=np.uint8)
    refused("not device memory", 8, (host.ctypes.data + 15) // 16 * 16, PLEN, ia, [8], ra, 8)   # a host address
    seg = next(x for x in torch.cuda.memory_snapshot() if x["address"] <= pa < x["address"] + x["total_size"])
    refused("past the pointer's allocation", 2, seg["address"] + seg["total_size"] - PLEN, PLEN, ia, [8], ra, 2)   # too small for its allocation
    refused("past the pointer's allocation", 8, pa, seg["total_size"] // 4 // 16 * 16, ia, [8], ra, 8)
    refused("column count", 8, pa, PLEN + 64, ia, [4, 4], ra, 8)                            # a wrong column count
    refused("n_tail < n", 8, pa, PLEN + 64, ia, [8], ra, 7)
    refused("capacity", 9, pa, PLEN + 64, ia, [8], ra, 9)
    # the Python mirror refuses what it can see before the library is reached, and a tensor that does not hold the rows
    with pytest.raises(ValueError, match="16-byte aligned"):
        b.upload_device(pa + 8, 7, PLEN + 64, ia, [8], ra, 7)
    with pytest.raises(ValueError, match="must hold 8 rows"):
        b.upload_tensors(proofs, insts[:7], [8], draws)
    with pytest.raises(TypeError, match="uint8"):
        b.upload_tensors(proofs.to(torch.int16), insts, [8], draws)
    with pytest.raises(ValueError, match="context's device"):
        b.upload_tensors(proofs.cpu(), insts, [8], draws)
    # the batch still works
    b.upload_device(pa, 8, PLEN + 64, ia, [8], ra, 8)
    b.launch()
    assert b.finish_groups() == want
    b.close()


# The refusals every upload shares, whatever its source: (name, set_groups / set_group_sizes first, the call's changes, code, message,
# entry points).  Codes and texts are those of include/h2v.h and of the three entry points before they shared their checks:
# H2V_ERR_BAD_ARGUMENT -16 everywhere but the host forms' column count, the reference's own H2V_ERR_INVALID_INSTANCES -1.
HOST_FORMS, ALL_FORMS = ("upload", "upload_launch"), ("upload", "upload_launch", "upload_device")
SHARED_REFUSALS = [
    ("capacity", None, dict(n=9, nt=9), -16, "capacity", ALL_FORMS),
    ("columns_host", None, dict(cols=[4, 4]), -1, "column count", HOST_FORMS),
    ("columns_device", None, dict(cols=[4, 4]), -16, "column count", ("upload_device",)),
    ("short_tail", None, dict(nt=7), -16, "n_tail < n", ALL_FORMS),
    ("group_multiple", 4, dict(n=6, nt=6), -16, "multiples of the group count", ALL_FORMS),
    ("group_sum", [1, 7], dict(n=7, nt=7), -16, "sum of the group sizes", ALL_FORMS),
    ("group_draws", [1, 7], dict(nt=9), -16, "one draw per proof", ALL_FORMS),
    ("no_instances", None, dict(instances=False), -16, "instances missing", ALL_FORMS),
    ("no_col_lens", None, dict(col_lens=False), -16, "null argument", ALL_FORMS),
    ("short_proof_len", None, dict(proof_len=PLEN - 1), -16, "proof_len is shorter", HOST_FORMS),
    ("draw_of_r", None, dict(first_draw=R_MOD), -16, "rand32 scalar not canonical", HOST_FORMS),
]


@pytest.mark.parametrize("form", ALL_FORMS)
def test_shared_refusals_through_every_entry_point(pool, ctx, form):
    """raw calls of h2v_batch_upload, h2v_batch_upload_launch and h2v_batch_upload_device with one argument wrong at a time: the code,
    the text, a batch left Empty; then a valid upload through the same entry point equals the host run"""
    import torch
    import halo2_verifier_amd as h2v
    s, P, I = pool
    rand = _draws(9, 31)                       # (a ninth draw for the tail that is one too long)
    want = _host(ctx, P[:8], I[:8], rand[:8])
    assert want[0] == [True] and want[1] == [0] * 8
    flat, inst = _flat(P[:8], I[:8])
    proofs, insts, draws = _tensors(P[:8], I[:8], rand)
    torch.cuda.synchronize()
    b = _batch(ctx, 8)
    lib, sz = b._lib, h2v.verifier._sizes

    def call(n=8, nt=8, cols=(8,), instances=True, col_lens=True, proof_len=PLEN, first_draw=None):
        cl = sz(list(cols)) if col_lens else None
        ncols = len(cols)
        if form == "upload_device":
            vp = ctypes.c_void_p
            return lib.h2v_batch_upload_device(b._h, n, vp(proofs.data_ptr()), PLEN, vp(insts.data_ptr() if instances else 0), ncols, cl, vp(draws.data_ptr()), nt)
        tail = _rand_bytes(([first_draw] if first_draw is not None else rand[:1]) + rand[1:])
        args = (b._h, n, flat, proof_len, inst if instances else None, ncols, cl, tail, nt)
        return lib.h2v_batch_upload(*args) if form == "upload" else lib.h2v_batch_upload_launch(*args, 1)

    ran = []
    for name, groups, changes, code, text, forms in SHARED_REFUSALS:
        if form not in forms:
            continue
        if isinstance(groups, list):
            b.set_group_sizes(groups)
        else:
            b.set_groups(groups or 1)
        assert call(**changes) == code, (name, h2v._lib.last_error())
        assert text in h2v._lib.last_error(), (name, h2v._lib.last_error())
        with pytest.raises(h2v.H2VError, match="nothing uploaded"):
            b.launch()
        ran.append(name)
    assert len(ran) == (10 if form != "upload_device" else 8)
    b.set_groups(1)
    assert call() == 0, h2v._lib.last_error()
    b.n = 8
    if form != "upload_launch":
        b.launch()
    assert b.finish_groups() == want
    b.close()


def test_unequal_groups_reach_the_device_by_set_group_sizes_alone(pool, ctx):
    """one object: unequal sizes, other unequal sizes, equal groups, a host upload of the same proofs and draws each time.  No upload
    sends the offsets or the last-of-group marks: a stale device copy of either would give another group's channels"""
    s, P, I = pool
    rand = _draws(8, 37)
    flat, inst = _flat(P[:8], I[:8])
    b = _batch(ctx, 8)
    seen = []
    for groups, sizes in ((1, [1, 7]), (1, [5, 3]), (2, None)):
        if sizes:
            b.set_group_sizes(sizes)
        else:
            b.set_groups(groups)
        b.upload(flat, PLEN, inst, [8], _rand_bytes(rand)); b.launch()
        got = b.finish_groups()
        assert got[0] == [True, True] and got[1] == [0] * 8
        assert got == _host(ctx, P[:8], I[:8], rand, groups, sizes), (groups, sizes)
        seen.append(got)
    assert seen[0][2:] != seen[1][2:] and seen[1][2:] != seen[2][2:]     # (the shapes do differ in what they accumulate)
    b.close()


def test_a_draw_of_r_is_reported_by_finish(pool, ctx):
    import torch
    import halo2_verifier_amd as h2v
    s, P, I = pool
    rand = _draws(16, 19)
    want = _host(ctx, P[:16], I[:16], rand, 4)
    bad = list(rand)
    bad[9], bad[13] = R_MOD + 1, R_MOD
    b = _batch(ctx, 16, 4)
    proofs, insts, draws = _tensors(P[:16], I[:16], bad)
    b.upload_tensors(proofs, insts, [8], draws)
    b.launch()
    with pytest.raises(h2v.H2VError, match="draw 9 ") as e:
        b.finish_groups()
    assert e.value.code == -16
    with pytest.raises(h2v.H2VError, match="nothing uploaded"):
        b.launch()
    with pytest.raises(h2v.H2VError):
        b.finish_groups()
    proofs, insts, draws = _tensors(P[:16], I[:16], rand)
    torch.cuda.synchronize()
    b.upload_device(proofs.data_ptr(), 16, PLEN, insts.data_ptr(), [8], draws.data_ptr(), 16)
    b.launch()
    assert b.finish_groups() == want
    b.close()


@pytest.mark.parametrize("shape", ["equal", "unequal"])
def test_no_host_wait_behind_a_busy_stream(pool, ctx, shape):
    """about a second of spinning is queued on the batch's stream: upload_device with device draws returns while it still runs"""
    import torch
    s, P, I = pool
    groups, sizes = (4, None) if shape == "equal" else (1, [1, 7, 5, 3])
    rand = _draws(16, 23)
    want = _host(ctx, P[:16], I[:16], rand, groups, sizes)
    proofs, insts, draws = _tensors(P[:16], I[:16], rand, PLEN + 16)
    b = _batch(ctx, 16, groups, sizes)
    args = (proofs.data_ptr(), 16, PLEN + 16, insts.data_ptr(), [8], draws.data_ptr(), 16)
    torch.cuda.synchronize()
    b.upload_device(*args); b.launch()                 # the warm call: every buffer has its size, the plan is compiled
    assert b.finish_groups() == want
    stream = torch.cuda.ExternalStream(b.stream, device="cuda:0")
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):                    # how long 10^7 of _sleep's cycles take here
        t0.record(); torch.cuda._sleep(10_000_000); t1.record()
    t1.synchronize()
    cycles = int(10_000_000 * 1000.0 / max(t0.elapsed_time(t1), 1e-3))
    behind = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        behind.record()
    began = time.perf_counter()
    b.upload_device(*args)
    took = time.perf_counter() - began
    assert not behind.query(), f"upload_device returned after {took:.3f} s, when the stream's earlier work was done"
    b.launch()
    assert b.finish_groups() == want
    b.close()
