"""The enqueued feed of a resident accumulator (include/h2v_feed.h): Accumulator.feed(batch) behind a launch, Accumulator.settle()
whenever the caller wants the host's books up to date.

The definition under test: feed(b); settle() equals process_batch(b) after a host finish of the same launch — the TWIN, a second
accumulator fed that way from the same batch object, which also shows that the feed left the batch as it was — and that equals
process() once per group.  Every comparison is of bytes and integers: read()'s affine points and counters, check_legs()' rows,
finalize(), and read() again after a drop_legs().  The toy key and the 24-proof pool are test_gpu_accumulator_batch.py's.

Cases 1 to 7 need the entry points and fail without them."""
import ctypes
import random
import time

import pytest

import batch_reference
import circuits
import feed_reference
from circuits import R_MOD

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = -16, -19
ACC_BYTES = 1312


def _ctx(s, device=0):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript, circuit_instances=s.circuit_instances, device=device)


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


def _rand_bytes(rand):
    return b"".join(r.to_bytes(32, "little") for r in rand)


def _slices(sizes):
    out, at = [], 0
    for sz in sizes:
        out.append(slice(at, at + sz)); at += sz
    return out


def _flat(P, I):
    return b"".join(P), b"".join(v for inst in I for col in inst for v in col)


def _launch(ctx, P, I, rand, sizes, pairing=True, equal=False, batch=None):
    """upload + launch of the proofs in groups of `sizes` (equal=True: through set_groups) -> the batch, Launched"""
    import halo2_verifier_amd as h2v
    col_lens = [len(col) for col in I[0]]
    b = batch if batch is not None else h2v.Batch(ctx, len(P), sum(col_lens))
    if equal:
        assert len(set(sizes)) == 1
        b.set_groups(len(sizes))
    else:
        b.set_group_sizes(sizes)
    flat, inst = _flat(P, I)
    b.upload(flat, len(P[0]), inst, col_lens, _rand_bytes(rand))
    b.launch(with_pairing=pairing)
    return b


def _launch_tensors(ctx, P, I, draw_bytes, sizes, pairing=True, batch=None):
    """the same from device tensors, the draws included (h2v_batch_upload_device: nothing here waits for the batch's stream)"""
    import torch
    import halo2_verifier_amd as h2v
    col_lens = [len(col) for col in I[0]]
    b = batch if batch is not None else h2v.Batch(ctx, len(P), sum(col_lens))
    if batch is None:
        b.set_group_sizes(sizes)
    flat, inst = _flat(P, I)
    n = len(P)
    proofs = torch.frombuffer(bytearray(flat), dtype=torch.uint8).reshape(n, len(P[0])).cuda()
    insts = torch.frombuffer(bytearray(inst), dtype=torch.uint8).reshape(n, len(inst) // n).cuda()
    draws = torch.frombuffer(bytearray(draw_bytes), dtype=torch.uint8).reshape(len(draw_bytes) // 32, 32).cuda()
    b.upload_tensors(proofs, insts, col_lens, draws)
    b.launch(with_pairing=pairing)
    return b


def _by_process(ctx, P, I, rand, sizes, acc):
    st = []
    for sl in _slices(sizes):
        st += acc.process(ctx, None, P[sl], I[sl], rand[sl])
    return st


def _state(acc):
    return acc.read(), acc.check_legs(), acc.finalize()


def _cycled(P, I, n):
    return [P[i % len(P)] for i in range(n)], [I[i % len(I)] for i in range(n)]


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 24, seed=555, threads=8)
    ctx = _ctx(s)
    yield s, P, I, ctx
    ctx.close()
    s.free()


def _led(ctx, P, I, journal, k=3):
    """k accumulators with the same two proofs processed: a non-trivial (L, R) and one journal entry in front of what the test feeds"""
    import halo2_verifier_amd as h2v
    lead = _draws(2, 8)
    accs = [h2v.Accumulator(ctx, journal=journal) for _ in range(k)]
    for a in accs:
        assert a.process(ctx, None, P[22:24], I[22:24], lead) == [0, 0]
    return accs


SHAPES = {"one_proof": ([1], True), "4x4": ([4] * 4, True), "unequal": ([1, 5, 2, 8], False)}


# ---- 1. one feed against a twin
@pytest.mark.parametrize("finished", [False, True], ids=["launched", "finished"])
@pytest.mark.parametrize("pairing", [True, False], ids=["pairing", "no_pairing"])
@pytest.mark.parametrize("name", list(SHAPES))
def test_one_feed_against_a_twin(pool, name, pairing, finished):
    s, P, I, ctx = pool
    sizes, equal = SHAPES[name]
    n, G = sum(sizes), len(sizes)
    rand = _draws(n, 100 + n + G)
    fed, twin, ref = _led(ctx, P, I, G + 2)
    b = _launch(ctx, P[:n], I[:n], rand, sizes, pairing=pairing, equal=equal)
    if finished:
        first = b.finish_groups()
    assert fed.pending == (0, 0)
    assert fed.feed(b) is None
    assert fed.pending == (1, 1)
    assert fed.settle() == [(0, n, 0)]
    assert fed.pending == (0, 0) and fed.settle() == []
    fin = b.finish_groups()                                  # the batch was only read: its own finish is what it would have been
    assert fin[0] == [True] * G and fin[1] == [0] * n
    if finished:
        assert fin == first
    assert twin.process_batch(b) == (n, 0)
    assert _by_process(ctx, P[:n], I[:n], rand, sizes, ref) == [0] * n
    want = _state(twin)
    assert _state(fed) == want == _state(ref)
    assert want[1] == [(0, 0, True), (2, 0, True)] + [(sz, 0, True) for sz in sizes] and want[2][0] is True
    exp = batch_reference.expected([(s, p, i) for p, i in zip(P[22:24] + P[:n], I[22:24] + I[:n])], _draws(2, 8) + rand)
    assert want[0] == (exp[2], exp[3], n + 2, 0)
    # drop_legs afterwards: the journal a feed left rebuilds the points as the twin's does
    for a in (fed, twin, ref):
        a.drop_legs([1] if G == 1 else [1, 3])
    assert _state(fed) == _state(twin) == _state(ref)
    assert len(fed._inputs) == len(twin._inputs) == len(fed.check_legs())
    for a in (fed, twin, ref):
        a.close()
    b.close()


# ---- 2. 512 groups of one proof: the t + 1 < LEG_WEIGHTS_MAX edge of the weights
def test_512_groups_of_one_proof(pool):
    s, P24, I24, ctx = pool
    n = 512
    P, I = _cycled(P24, I24, n)
    rand = _draws(n, 512)
    fed, twin = _led(ctx, P24, I24, n + 2, k=2)
    b = _launch(ctx, P, I, rand, [1] * n, pairing=False, equal=True)
    fed.feed(b)
    assert fed.settle() == [(0, n, 0)]
    assert b.finish_groups()[1] == [0] * n
    assert twin.process_batch(b) == (n, 0)
    want = _state(twin)
    assert _state(fed) == want
    assert want[0][2:] == (n + 2, 0) and want[2][0] is True and len(want[1]) == n + 2 and all(row[2] for row in want[1])
    # the last group's weight is the 1 the kernel takes where the scan has no element: dropping the last leg is dropping its own sum
    fed.drop_legs([n + 1]); twin.drop_legs([n + 1])
    assert _state(fed) == _state(twin)
    fed.close(); twin.close(); b.close()


# ---- 3. several feeds before one settle
@pytest.mark.parametrize("implicit", [False, True], ids=["settle", "read_settles"])
def test_three_feeds_of_two_batches_before_one_settle(pool, implicit):
    s, P, I, ctx = pool
    r1, r2 = _draws(6, 31), _draws(7, 32)
    fed, twin = _led(ctx, P, I, 12, k=2)
    b1 = _launch(ctx, P[:6], I[:6], r1, [2, 4])
    b2 = _launch(ctx, P[6:13], I[6:13], r2, [3, 1, 3], pairing=False)
    fed.feed(b1); fed.feed(b2); fed.feed(b1)                 # no call in between; the same launch may be fed again
    assert fed.pending == (3, 3) and len(fed._inputs) == 2
    if implicit:
        got = fed.read()                                     # every other call settles first
        assert fed.pending == (0, 3)                         # ... and the reports wait for settle()
    assert fed.settle() == [(0, 6, 0), (0, 7, 0), (0, 6, 0)]
    assert fed.pending == (0, 0) and fed.settle() == []
    b1.finish_groups(); b2.finish_groups()
    for b in (b1, b2, b1):
        twin.process_batch(b)
    want = _state(twin)
    assert _state(fed) == want
    if implicit:
        assert got == want[0]
    assert [row[:2] for row in want[1]] == [(0, 0), (2, 0)] + [(k, 0) for k in (2, 4, 3, 1, 3, 2, 4)]
    assert want[0][2:] == (21, 0) and len(fed._inputs) == len(twin._inputs) == 9
    fed.drop_legs([2, 5, 8]); twin.drop_legs([2, 5, 8])
    assert _state(fed) == _state(twin)
    fed.close(); twin.close(); b1.close(); b2.close()


# ---- 4. test_gpu_accumulator_batch.py's failing cases through the feed
def test_a_proof_failing_by_status(pool):
    s, P, I, ctx = pool
    rand = _draws(12, 6)
    bad = list(P[:12])
    x = bytearray(bad[7]); x[-33] = 0xff; bad[7] = bytes(x)      # an undecodable opening point, in group 2
    exp = circuits.oracle_verify_batch(s, bad, I[:12], rand)
    assert exp[0] is False and [i for i, v in enumerate(exp[1]) if v] == [7]
    sizes = [4, 2, 5, 1]
    import halo2_verifier_amd as h2v
    fed, ref = h2v.Accumulator(ctx, journal=8), h2v.Accumulator(ctx, journal=8)
    b = _launch(ctx, bad, I[:12], rand, sizes)
    fed.feed(b)
    assert fed.settle() == [(0, 12, 1)]                          # counted from the device's status words
    assert b.finish_groups()[1] == exp[1]
    assert _by_process(ctx, bad, I[:12], rand, sizes, ref) == exp[1]
    assert fed.read() == ref.read() == (exp[2], exp[3], 12, 1)
    assert fed.finalize() == ref.finalize() == (False, exp[2], exp[3])
    assert fed.check_legs() == ref.check_legs() == [(0, 0, True), (4, 0, True), (2, 0, True), (5, 1, True), (1, 0, True)]
    fed.close(); ref.close(); b.close()


def test_a_pairing_only_bad_proof_is_found_and_dropped(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    sizes = [3, 5, 6, 2]
    sl = _slices(sizes)
    rand = _draws(16, 7)
    I2 = list(I[:16])
    at = sl[2].start + 4
    I2[at] = [[circuits.le32(5)] + I[at][0][1:]]                 # a wrong public input: every status 0, the pairing fails
    lead = _draws(2, 8)
    acc = h2v.Accumulator(ctx, journal=8)
    assert acc.process(ctx, None, P[16:18], I[16:18], lead) == [0, 0]
    b = _launch(ctx, P[:16], I2, rand, sizes, pairing=False)
    acc.feed(b)
    assert acc.settle() == [(0, 16, 0)]
    whole = batch_reference.expected([(s, p, i) for p, i in zip(P[16:18] + P[:16], I[16:18] + I2)], lead + rand)
    assert acc.finalize() == (False, whole[2], whole[3])
    assert acc.check_legs() == [(0, 0, True), (2, 0, True), (3, 0, True), (5, 0, True), (6, 0, False), (2, 0, True)]
    fin = b.finish_groups()
    st, own, _ = b.identify()                                    # the still-resident batch names the proof
    assert [i for i, v in enumerate(st) if v] == [at] and own == [True, True, False, True]
    assert b.finish_groups() == fin
    acc.drop_legs([4])
    keep = [i for i in range(16) if not sl[2].start <= i < sl[2].stop]
    want = batch_reference.expected([(s, p, i) for p, i in zip(P[16:18], I[16:18])] + [(s, P[i], I2[i]) for i in keep], lead + [rand[i] for i in keep])
    assert want[0] is True
    assert acc.read() == (want[2], want[3], 12, 0) and acc.finalize() == (True, want[2], want[3])
    assert acc.check_legs() == [(0, 0, True), (2, 0, True), (3, 0, True), (5, 0, True), (2, 0, True)]
    acc.close(); b.close()


# ---- 5. a draw >= r in a tail uploaded from device memory: the feed fails closed
def test_a_draw_not_below_r_drops_the_feed_on_the_device(pool):
    s, P, I, ctx = pool
    model = feed_reference.Model(capacity=8)
    fed, twin = _led(ctx, P, I, 8, k=2)
    model.process_batch([2])
    before = _state(fed)
    assert before[2][0] is True
    sizes, n = [2, 3, 1, 4], 10
    tail = bytearray(_rand_bytes(_draws(n, 51)))
    tail[32 * 6:32 * 7] = R_MOD.to_bytes(32, "little")          # the bytes of r as draw 6
    bad = _launch_tensors(ctx, P[:n], I[:n], bytes(tail), sizes)
    fed.feed(bad)
    model.feed(sizes)
    assert fed.settle() == model.settle([(BAD_ARGUMENT, None)]) == [(BAD_ARGUMENT, n, n)]
    after = _state(fed)
    assert after[0][:2] == before[0][:2]                        # the points keep their value
    assert after[0][2:] == (2 + n, n) == (model.n_proofs, model.n_failed)   # both counters grow by n
    assert after[1] == before[1] and [row[:2] for row in after[1]] == model.legs()   # no journal entry
    assert after[2] == (False, before[2][1], before[2][2])      # finalize is not ok, over the same points
    # a good feed enqueued behind a dropped one, in the same settle, is committed
    rand = _draws(5, 52)
    good = _launch(ctx, P[10:15], I[10:15], rand, [2, 3])
    fed.feed(bad); fed.feed(good)
    model.feed(sizes); model.feed([2, 3])
    assert fed.pending == model.pending == (2, 2)
    assert fed.settle() == model.settle([(BAD_ARGUMENT, None), (0, [0, 0])]) == [(BAD_ARGUMENT, n, n), (0, 5, 0)]
    good.finish_groups()
    assert twin.process_batch(good) == (5, 0)
    tw = _state(twin)
    got = _state(fed)
    assert got[0][:2] == tw[0][:2] and got[0][2:] == (2 + 2 * n + 5, 2 * n) == (model.n_proofs, model.n_failed)
    assert got[1] == tw[1] and [row[:2] for row in got[1]] == model.legs()
    assert got[2] == (False, tw[2][1], tw[2][2]) and tw[2][0] is True
    # the free slots are as before: 4 entries in use, 4 free — five groups do not fit, four do, into the slots the twin's take
    assert len(model.free) == 4
    five = _launch(ctx, P[:5], I[:5], _draws(5, 53), [1] * 5, equal=True)
    with pytest.raises(Exception, match="journal"):
        fed.feed(five)
    four = _launch(ctx, P[:4], I[:4], _draws(4, 54), [1] * 4, equal=True)
    fed.feed(four)
    assert fed.settle() == [(0, 4, 0)]
    four.finish_groups()
    twin.process_batch(four)
    assert _state(fed)[1] == _state(twin)[1] and fed.read()[:2] == twin.read()[:2]
    fed.drop_legs([2]); twin.drop_legs([2])                      # the rebuilt points agree: every entry sits in the slot its sum went to
    assert fed.read()[:2] == twin.read()[:2] and fed.check_legs() == twin.check_legs()
    for o in (fed, twin, bad, good, five, four):
        o.close()


def _sleep_cycles(stream, seconds):
    """how many of torch.cuda._sleep's cycles take `seconds` on this stream's device"""
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):
        t0.record(); torch.cuda._sleep(10_000_000); t1.record()
    t1.synchronize()
    return int(10_000_000 * 1000.0 * seconds / max(t0.elapsed_time(t1), 1e-3))


# ---- 6. no host wait (test_gpu_device_finish.py::test_no_host_wait_behind_a_busy_stream's recipe)
def test_no_host_wait_behind_a_busy_stream(pool):
    """about a second of spinning is queued on the batch's stream behind a launch: feed returns while it still runs"""
    import torch
    s, P, I, ctx = pool
    sizes, n = [4] * 4, 16
    rand = _draws(n, 61)
    fed, twin = _led(ctx, P, I, 12, k=2)
    b = _launch(ctx, P[:n], I[:n], rand, sizes, equal=True)
    fed.feed(b)                                               # the warm call: the scratch, the pinned block and the events exist
    assert fed.settle() == [(0, n, 0)]
    stream = torch.cuda.ExternalStream(b.stream, device="cuda:0")
    cycles = _sleep_cycles(stream, 1.0)
    b.launch()
    behind = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        behind.record()
    began = time.perf_counter()
    fed.feed(b)
    took = time.perf_counter() - began
    assert not behind.query(), f"feed returned after {took:.3f} s, when the stream's earlier work was done"
    assert fed.pending == (1, 1)
    assert fed.settle() == [(0, n, 0)]                        # (this one waits: the feed ran behind the sleep)
    assert behind.query()
    b.finish_groups()
    twin.process_batch(b); twin.process_batch(b)
    assert _state(fed) == _state(twin)
    fed.close(); twin.close(); b.close()


# ---- 7. the batch uploaded again under a pending feed
def test_the_batch_is_uploaded_again_under_a_pending_feed(pool):
    """Launch, a sleep on the batch's stream, feed — and at once other proofs into the same batch, launch, feed.  Both sets of legs
    equal the twin's.  This shows that the ordering (the accumulator's stream behind the batch's, the batch's next upload behind the
    feed's read event) holds in THIS schedule; it does not show that a race is absent."""
    import torch
    s, P, I, ctx = pool
    sizes, n = [3, 1, 4], 8
    r1, r2 = _draws(n, 71), _draws(n, 72)
    fed, twin = _led(ctx, P, I, 12, k=2)
    b = _launch_tensors(ctx, P[:n], I[:n], _rand_bytes(r1), sizes, pairing=False)
    stream = torch.cuda.ExternalStream(b.stream, device="cuda:0")
    cycles = _sleep_cycles(stream, 0.2)
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
    fed.feed(b)
    _launch_tensors(ctx, P[n:2 * n], I[n:2 * n], _rand_bytes(r2), sizes, batch=b)      # nothing of it waits for the stream
    fed.feed(b)
    assert fed.pending == (2, 2)
    assert fed.settle() == [(0, n, 0), (0, n, 0)]
    tb = _launch(ctx, P[:n], I[:n], r1, sizes, pairing=False)
    tb.finish_groups()
    twin.process_batch(tb)
    _launch(ctx, P[n:2 * n], I[n:2 * n], r2, sizes, batch=tb)
    tb.finish_groups()
    twin.process_batch(tb)
    want = _state(twin)
    assert _state(fed) == want and want[2][0] is True
    exp = batch_reference.expected([(s, p, i) for p, i in zip(P[22:24] + P[:2 * n], I[22:24] + I[:2 * n])], _draws(2, 8) + r1 + r2)
    assert want[0] == (exp[2], exp[3], 2 * n + 2, 0)
    assert b.finish_groups()[1] == [0] * n
    fed.close(); twin.close(); b.close(); tb.close()


# ---- 8. refusals change nothing
def _raw(acc_h, batch_h):
    from halo2_verifier_amd import _lib, feed
    rc = feed._library().h2v_accumulator_feed_batch(acc_h, batch_h)
    return rc, _lib.last_error() if rc else ""


def test_refusals_change_nothing(pool):
    import torch
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    rand = _draws(8, 9)
    acc, twin = _led(ctx, P, I, 6, k=2)
    before = (acc.read(), acc.check_legs())

    def refused(batch, code, word, fin=None, pending=(0, 0)):
        rc, msg = _raw(acc._h, batch._h if batch is not None else None)
        assert rc == code and word in msg, (rc, msg)
        assert acc.pending == pending
        if pending == (0, 0):
            assert (acc.read(), acc.check_legs()) == before
        if fin is not None:
            assert batch.finish_groups() == fin

    refused(None, BAD_ARGUMENT, "null")
    rc, msg = _raw(None, None)
    assert rc == BAD_ARGUMENT and "null" in msg
    # stage Empty, then Uploaded
    b = h2v.Batch(ctx, 8, 8)
    refused(b, BAD_ARGUMENT, "launch")
    b.set_groups(2)
    flat, inst = _flat(P[:8], I[:8])
    b.upload(flat, len(P[0]), inst, [8], _rand_bytes(rand))
    refused(b, BAD_ARGUMENT, "launch")
    # after a fold
    b.launch(with_pairing=False)
    rec = torch.zeros(2 * ACC_BYTES, dtype=torch.uint8, device="cuda:0")
    b.export_accumulators(rec.data_ptr())
    b.fold_check_enqueue(rec.data_ptr(), 1)
    refused(b, BAD_ARGUMENT, "fold")
    fin_b = b.finish_groups()
    assert fin_b[0] == [True, True]
    refused(b, BAD_ARGUMENT, "fold", fin_b)
    # a shard: a tail of draws longer than the upload
    b.set_groups(1)
    b.upload(flat, len(P[0]), inst, [8], _rand_bytes(rand + _draws(4, 11)))
    b.launch(with_pairing=False)
    refused(b, BAD_ARGUMENT, "shard")
    b.close()
    # another params
    other = circuits.setup_vector_mul(8, 8, s_seed=43)
    Po, Io = circuits.prove_vector_mul_batch(other, 2, seed=5, threads=2)
    co = _ctx(other)
    bo = _launch(co, Po, Io, rand[:2], [1, 1])
    refused(bo, BAD_ARGUMENT, "params")
    assert bo.finish_groups()[0] == [True, True]
    bo.close(); co.close(); other.free()
    # a full journal, the legs of the feeds still pending counted: 2 entries, 2 pending legs, a batch of 3 groups, capacity 6
    good = _launch(ctx, P[:8], I[:8], rand, [4, 4], equal=True)
    three = _launch(ctx, P[8:14], I[8:14], rand[:6], [1, 2, 3])
    acc.feed(good)
    refused(three, UNSUPPORTED, "journal", pending=(1, 1))
    assert acc.settle() == [(0, 8, 0)]
    good.finish_groups()
    twin.process_batch(good)
    assert _state(acc) == _state(twin)
    before = (acc.read(), acc.check_legs())
    refused(three, UNSUPPORTED, "journal")                     # 4 entries + 3 > 6 as well
    two = _launch(ctx, P[8:14], I[8:14], rand[:6], [3, 3], equal=True, batch=three)
    acc.feed(two)                                              # ... and two groups fill the journal exactly
    assert acc.settle() == [(0, 6, 0)]
    two.finish_groups()
    twin.process_batch(two)
    assert _state(acc) == _state(twin) and len(acc.check_legs()) == 6
    # the Python mirror's own refusals
    with pytest.raises(TypeError):
        acc.feed(ctx)
    keeper = h2v.Accumulator(ctx, journal=8, keep_inputs=True)
    with pytest.raises(ValueError, match="Batch.identify"):
        keeper.feed(good)
    assert keeper.pending == (0, 0)
    for o in (keeper, acc, twin, good, three):
        o.close()


def test_the_65th_unreported_feed_is_refused(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    acc, twin = h2v.Accumulator(ctx), h2v.Accumulator(ctx)       # journal off: the limit is the reports'
    b = _launch(ctx, P[:2], I[:2], _draws(2, 65), [2], pairing=False)
    for _ in range(feed_reference.FEED_MAX_PENDING):
        acc.feed(b)
    assert acc.pending == (64, 64)
    rc, msg = _raw(acc._h, b._h)
    assert rc == UNSUPPORTED and "H2V_FEED_MAX_PENDING" in msg and acc.pending == (64, 64)
    got = acc.read()                                             # settled on the way, not reported: still refused
    assert acc.pending == (0, 64) and got[2:] == (128, 0)
    rc, msg = _raw(acc._h, b._h)
    assert rc == UNSUPPORTED and acc.pending == (0, 64) and acc.read() == got
    assert acc.settle() == [(0, 2, 0)] * 64
    acc.feed(b)
    assert acc.settle() == [(0, 2, 0)]
    b.finish_groups()
    for _ in range(65):
        twin.process_batch(b)
    assert acc.read() == twin.read() and acc.finalize() == twin.finalize() and acc.finalize()[0] is True
    acc.close(); twin.close(); b.close()


# ---- 9. one other instantiation: GWC + Keccak-256, two circuit instances per proof
def test_gwc_keccak_two_circuit_instances():
    s = circuits.setup_vector_mul(8, 6).set_options(circuits.GWC, circuits.KECCAK256).set_circuit_instances(2)
    pairs = [circuits.prove_vector_mul_multi(s, 2, seed=100 + i, rng_seed=7 + i) for i in range(9)]
    P, I = [p for p, _ in pairs], [i for _, i in pairs]
    ctx = _ctx(s)
    import halo2_verifier_amd as h2v
    rand = _draws(9, 17)
    sizes = [4, 1, 4]
    exp = circuits.oracle_verify_batch(s, P, I, rand)
    assert exp[0] is True
    fed, twin, ref = (h2v.Accumulator(ctx, journal=5) for _ in range(3))
    b = _launch(ctx, P, I, rand, sizes)
    fed.feed(b)
    assert fed.settle() == [(0, 9, 0)]
    b.finish_groups()
    assert twin.process_batch(b) == (9, 0)
    assert _by_process(ctx, P, I, rand, sizes, ref) == [0] * 9
    assert _state(fed) == _state(twin) == _state(ref)
    assert fed.read() == (exp[2], exp[3], 9, 0) and fed.finalize() == (True, exp[2], exp[3])
    for o in (fed, twin, ref, b, ctx):
        o.close()
    s.free()
