"""Feeding a finished staged batch to the resident accumulator (h2v_accumulator_process_batch): the G groups of the batch as G legs.

Group g holds the proofs [first_g, first_g + n_g) with draws r_{g,0} ..; S_g is the sum the launch left for it and M_g the product of
its draws:

    (L, R) <- (prod_g M_g) (L, R) + sum_g W_g S_g,     W_g = prod_{f > g} M_f

which is what h2v_accumulator_process called once per group leaves, and so ONE accumulation over all proofs so far with all draws
concatenated.  Expected values: the CPU oracle's one accumulation (circuits.oracle_verify_batch / oracle_accumulate,
batch_reference.expected) and `process` group by group on a second accumulator — points, counters, verdict, and with the journal on
the entries.  Every test here fails without the entry point.

Two of the listed refusals cannot be provoked through the public interface and are not covered: multipliers that are not those of
the uploaded draws (only the scratch batches of h2v_verify_batch_shapes carry gathered multipliers) and a guard-variant upload (only
h2v_guard_msm's scratch batch is one).  A batch on another device is covered where a second GPU is visible."""
import ctypes
import random

import pytest

import batch_reference
import circuits
import oracle_lib
from circuits import R_MOD

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED = -16, -19
ZERO = bytes(64)
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


def _stage(ctx, P, I, rand, sizes, pairing=True, equal=False, batch=None):
    """upload + launch + finish_groups of the proofs in groups of `sizes` (equal=True: through set_groups) -> (batch, finish_groups())"""
    import halo2_verifier_amd as h2v
    col_lens = [len(col) for col in I[0]]
    b = batch if batch is not None else h2v.Batch(ctx, len(P), sum(col_lens))
    if equal:
        assert len(set(sizes)) == 1
        b.set_groups(len(sizes))
    else:
        b.set_group_sizes(sizes)
    b.upload(b"".join(P), len(P[0]), b"".join(v for inst in I for col in inst for v in col), col_lens, _rand_bytes(rand))
    b.launch(with_pairing=pairing)
    return b, b.finish_groups()


def _by_process(ctx, P, I, rand, sizes, acc):
    """`process` once per group on acc -> the statuses"""
    st = []
    for sl in _slices(sizes):
        st += acc.process(ctx, None, P[sl], I[sl], rand[sl])
    return st


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


GROUPS = {
    "4x6": ([6] * 4, True, True),
    "unequal": ([1, 7, 2, 14], False, True),
    "one_group": ([24], True, False),
    "24x1": ([1] * 24, False, False),
    "65x1": ([1] * 65, False, True),
    "512x1": ([1] * 512, True, False),
}


@pytest.mark.parametrize("name", list(GROUPS))
def test_groups_equal_one_accumulation_and_process_per_group(pool, name):
    import halo2_verifier_amd as h2v
    s, P24, I24, ctx = pool
    sizes, equal, pairing = GROUPS[name]
    n, G = sum(sizes), len(sizes)
    P, I = _cycled(P24, I24, n)
    rand = _draws(n, 1000 + n + G)
    exp = circuits.oracle_verify_batch(s, P, I, rand)
    assert exp[0] is True
    b, fin = _stage(ctx, P, I, rand, sizes, pairing=pairing, equal=equal)
    assert fin[1] == [0] * n
    fed, ref = h2v.Accumulator(ctx, journal=G + 1), h2v.Accumulator(ctx, journal=G + 1)
    assert fed.process_batch(b) == (n, 0) and fed.last_all_ok is True
    assert _by_process(ctx, P, I, rand, sizes, ref) == exp[1]
    assert fed.read() == ref.read() == (exp[2], exp[3], n, 0)
    assert fed.finalize() == ref.finalize() == (exp[0], exp[2], exp[3])
    legs = fed.check_legs()
    assert legs == ref.check_legs() == [(0, 0, True)] + [(sz, 0, True) for sz in sizes]
    assert b.finish_groups() == fin          # the batch was only read
    fed.close(); ref.close(); b.close()


def test_mixing_feeders_and_two_batches(pool):
    """process, a batch, process_guards, two batches in a row, process — one accumulation over everything, in order"""
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    rand = _draws(24, 2)
    exp = circuits.oracle_verify_batch(s, P, I, rand)
    assert exp[0] is True
    guards = []
    for p, i in zip(P[9:12], I[9:12]):
        rc, g = circuits.oracle_guard(s, p, i)
        assert rc == 0
        guards.append(((g["left_scalars"], g["left_bases"]), (g["right_scalars"], g["right_bases"])))
    acc = h2v.Accumulator(ctx, journal=16)
    assert acc.process(ctx, None, P[:3], I[:3], rand[:3]) == [0] * 3
    b1, _ = _stage(ctx, P[3:9], I[3:9], rand[3:9], [2, 4])
    assert acc.process_batch(b1) == (6, 0)
    acc.process_guards(guards, rand[9:12])
    b2, _ = _stage(ctx, P[12:18], I[12:18], rand[12:18], [3, 3], equal=True, pairing=False)
    assert acc.process_batch(b2) == (6, 0)
    _stage(ctx, P[18:23], I[18:23], rand[18:23], [5], batch=b1)     # the first batch, uploaded again right after its feed
    assert acc.process_batch(b1) == (5, 0)
    assert acc.process(ctx, None, P[23:], I[23:], rand[23:]) == [0]
    assert acc.read() == (exp[2], exp[3], 24, 0) and acc.finalize() == (True, exp[2], exp[3])
    assert acc.check_legs() == [(0, 0, True)] + [(k, 0, True) for k in (3, 2, 4, 3, 3, 3, 5, 1)]
    # the journal's invariant: rebuilding the points from the entries (their sums and the M_g read back from the device) changes nothing
    acc.drop_legs([])
    assert acc.read() == (exp[2], exp[3], 24, 0)
    acc.close(); b1.close(); b2.close()


def test_batches_of_two_keys():
    import halo2_verifier_amd as h2v
    s8, s4 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4)
    assert s8.params == s4.params
    P8, I8 = circuits.prove_vector_mul_batch(s8, 6, seed=31, threads=4)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 5, seed=32, threads=4)
    c8, c4 = _ctx(s8), _ctx(s4)
    rand = _draws(11, 3)
    items = [(s8, p, i) for p, i in zip(P8, I8)] + [(s4, p, i) for p, i in zip(P4, I4)]
    exp = circuits.oracle_accumulate(items, rand)
    assert exp[0] is True
    acc = h2v.Accumulator(c4)
    b8, _ = _stage(c8, P8, I8, rand[:6], [2, 3, 1])
    b4, _ = _stage(c4, P4, I4, rand[6:], [4, 1])
    assert acc.process_batch(b8) == (6, 0) and acc.process_batch(b4) == (5, 0)
    assert acc.finalize() == (True, exp[2], exp[3]) and acc.read()[2:] == (11, 0)
    acc.close(); b8.close(); b4.close()
    c8.close(); c4.close()
    s8.free(); s4.free()


@pytest.mark.parametrize("mo,tr,m", [(circuits.GWC, circuits.KECCAK256, 1), (circuits.SHPLONK, circuits.BLAKE2B, 2)])
def test_other_instantiations(mo, tr, m):
    import halo2_verifier_amd as h2v
    s = circuits.setup_vector_mul(8, 6).set_options(mo, tr).set_circuit_instances(m)
    if m == 1:
        P, I = circuits.prove_vector_mul_batch(s, 9, seed=77, threads=4)
    else:
        pairs = [circuits.prove_vector_mul_multi(s, m, seed=100 + i, rng_seed=7 + i) for i in range(9)]
        P, I = [p for p, _ in pairs], [i for _, i in pairs]
    ctx = _ctx(s)
    rand = _draws(9, 17)
    exp = circuits.oracle_verify_batch(s, P, I, rand)
    assert exp[0] is True
    b, _ = _stage(ctx, P, I, rand, [4, 1, 4])
    acc = h2v.Accumulator(ctx)
    assert acc.process_batch(b) == (9, 0)
    assert acc.finalize() == (True, exp[2], exp[3])
    acc.close(); b.close(); ctx.close()
    s.free()


def test_edge_scalars_through_single_proof_groups(pool):
    """A group of ONE proof whose draw is v has M_g = v: the weights kernel's products and the scale kernel's scalars, programmed."""
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    L_ = oracle_lib.load()
    # 1 and r - 1 against the same proof: the sums cancel, both points the identity
    d = _draws(1, 4)
    b, _ = _stage(ctx, [P[0]] * 2, [I[0]] * 2, d + [R_MOD - 1], [1, 1])
    assert batch_reference.expected([(s, P[0], I[0])] * 2, d + [R_MOD - 1]) == (True, [0, 0], ZERO, ZERO)
    acc = h2v.Accumulator(ctx)
    assert acc.process_batch(b) == (2, 0)
    assert acc.read() == (ZERO, ZERO, 2, 0) and acc.finalize() == (True, ZERO, ZERO)
    # ... and 1 as a draw on a non-empty accumulator: (L, R) + Guard
    _stage(ctx, P[1:3], I[1:3], [1, 1], [1, 1], batch=b)
    assert acc.process_batch(b) == (2, 0)
    exp = batch_reference.expected([(s, P[0], I[0])] * 2 + [(s, p, i) for p, i in zip(P[1:3], I[1:3])], d + [R_MOD - 1, 1, 1])
    assert acc.read() == (exp[2], exp[3], 4, 0)
    acc.close(); b.close()
    # a draw of 0 as a group's first, middle and last draw, in the first, a middle and the last group
    for at in (0, 1, 2, 3, 4, 5, 6, 8):
        rand = _draws(9, 50 + at)
        rand[at] = 0
        exp = batch_reference.expected([(s, p, i) for p, i in zip(P[:9], I[:9])], rand)
        assert exp[0] is True
        b, _ = _stage(ctx, P[:9], I[:9], rand, [3, 3, 3], equal=bool(at % 2))
        acc, ref = h2v.Accumulator(ctx), h2v.Accumulator(ctx)
        lead = _draws(2, 60)
        assert acc.process(ctx, None, P[9:11], I[9:11], lead) == ref.process(ctx, None, P[9:11], I[9:11], lead) == [0, 0]
        assert acc.process_batch(b) == (9, 0)
        _by_process(ctx, P[:9], I[:9], rand, [3, 3, 3], ref)
        want = batch_reference.expected([(s, p, i) for p, i in zip(P[9:11] + P[:9], I[9:11] + I[:9])], lead + rand)
        assert acc.read() == ref.read() == (want[2], want[3], 11, 0), at
        acc.close(); ref.close(); b.close()
    # every GLV edge scalar and every programmed value, one single-proof group each, in launches of up to 64 groups on one accumulator:
    # (L, R) <- v (L, R) + Guard_p per group, tracked as coefficients of the four distinct proofs' own Guards
    values = batch_reference.glv_edge_scalars() + batch_reference.programmed_values()
    assert len(values) > 100 and all(0 < v < R_MOD for v in values)
    singles = [batch_reference.single(s, P[j], I[j]) for j in range(4)]
    assert all(rc == 0 for rc, _, _ in singles)
    coef = [0, 0, 0, 0]
    acc = h2v.Accumulator(ctx)
    b = h2v.Batch(ctx, 64, 8)
    for lo in range(0, len(values), 64):
        chunk = values[lo:lo + 64]
        idx = [(lo + t) % 4 for t in range(len(chunk))]
        _stage(ctx, [P[j] for j in idx], [I[j] for j in idx], chunk, [1] * len(chunk), batch=b, pairing=False)
        assert acc.process_batch(b) == (len(chunk), 0)
        for j, v in zip(idx, chunk):
            coef = [c * v % R_MOD for c in coef]
            coef[j] = (coef[j] + 1) % R_MOD
        left, right, n, failed = acc.read()
        terms = [(c, k) for k, c in enumerate(coef) if c]
        exp_left = oracle_lib.g1_msm(L_, [c for c, _ in terms], [singles[k][1] for _, k in terms])
        exp_right = oracle_lib.g1_msm(L_, [c for c, _ in terms], [singles[k][2] for _, k in terms])
        assert (left, right, n, failed) == (exp_left, exp_right, lo + len(chunk), 0), lo
    ok, left, right = acc.finalize()
    assert ok is True and circuits.oracle_pairing_check(s, left, right)
    acc.close(); b.close()


def test_a_proof_failing_by_status(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    rand = _draws(12, 6)
    bad = list(P[:12])
    x = bytearray(bad[7]); x[-33] = 0xff; bad[7] = bytes(x)      # an undecodable opening point, in group 2
    exp = circuits.oracle_verify_batch(s, bad, I[:12], rand)
    assert exp[0] is False and [i for i, v in enumerate(exp[1]) if v] == [7]
    sizes = [4, 2, 5, 1]
    b, fin = _stage(ctx, bad, I[:12], rand, sizes)
    assert fin[1] == exp[1]
    acc, ref = h2v.Accumulator(ctx, journal=8), h2v.Accumulator(ctx, journal=8)
    assert acc.process_batch(b) == (12, 1) and acc.last_all_ok is False
    assert _by_process(ctx, bad, I[:12], rand, sizes, ref) == exp[1]
    assert acc.read() == ref.read() == (exp[2], exp[3], 12, 1)
    assert acc.finalize() == ref.finalize() == (False, exp[2], exp[3])
    assert acc.check_legs() == ref.check_legs() == [(0, 0, True), (4, 0, True), (2, 0, True), (5, 1, True), (1, 0, True)]
    acc.close(); ref.close(); b.close()


def test_a_pairing_only_bad_proof_is_found_and_dropped(pool):
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    sizes = [3, 5, 6, 2]
    sl = _slices(sizes)
    rand = _draws(16, 7)
    I2 = list(I[:16])
    at = sl[2].start + 4
    I2[at] = [[circuits.le32(5)] + I[at][0][1:]]                 # a wrong public input: every status 0, the pairing fails
    exp = circuits.oracle_verify_batch(s, P[:16], I2, rand)
    assert exp[0] is False and exp[1] == [0] * 16
    lead = _draws(2, 8)
    acc = h2v.Accumulator(ctx, journal=8)
    assert acc.process(ctx, None, P[16:18], I[16:18], lead) == [0, 0]
    b, fin = _stage(ctx, P[:16], I2, rand, sizes, pairing=False)
    assert acc.process_batch(b) == (16, 0)
    whole = batch_reference.expected([(s, p, i) for p, i in zip(P[16:18] + P[:16], I[16:18] + I2)], lead + rand)
    assert acc.finalize() == (False, whole[2], whole[3])
    legs = acc.check_legs()
    assert legs == [(0, 0, True), (2, 0, True), (3, 0, True), (5, 0, True), (6, 0, False), (2, 0, True)]
    # the still-resident batch names the proof
    st, own, _ = b.identify()
    assert [i for i, v in enumerate(st) if v] == [at] and own == [True, True, False, True]
    assert b.finish_groups() == fin
    # without the group: the accumulation over the other groups, the same draws
    acc.drop_legs([4])
    keep = [i for i in range(16) if not sl[2].start <= i < sl[2].stop]
    want = batch_reference.expected([(s, p, i) for p, i in zip(P[16:18], I[16:18])] + [(s, P[i], I2[i]) for i in keep], lead + [rand[i] for i in keep])
    assert want[0] is True
    assert acc.read() == (want[2], want[3], 12, 0) and acc.finalize() == (True, want[2], want[3])
    assert acc.check_legs() == [(0, 0, True), (2, 0, True), (3, 0, True), (5, 0, True), (2, 0, True)]
    acc.close(); b.close()


def _raw(acc_h, batch_h):
    from halo2_verifier_amd import _lib
    lib = _lib.load_library()
    n, f = ctypes.c_size_t(7), ctypes.c_size_t(7)
    rc = lib.h2v_accumulator_process_batch(acc_h, batch_h, ctypes.byref(n), ctypes.byref(f))
    return rc, _lib.last_error() if rc else ""


def test_refusals_change_nothing(pool):
    import torch
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    rand = _draws(8, 9)
    acc = h2v.Accumulator(ctx, journal=6)
    assert acc.process(ctx, None, P[8:10], I[8:10], _draws(2, 10)) == [0, 0]
    before = (acc.read(), acc.check_legs())

    def refused(batch, code, word, fin=None):
        rc, msg = _raw(acc._h, batch._h if batch is not None else None)
        assert rc == code and word in msg, (rc, msg)
        assert (acc.read(), acc.check_legs()) == before
        if fin is not None:
            assert batch.finish_groups() == fin

    good, fin = _stage(ctx, P[:8], I[:8], rand, [2, 2, 2, 2], equal=True)
    # a null argument
    refused(None, BAD_ARGUMENT, "null")
    rc, msg = _raw(None, good._h)
    assert rc == BAD_ARGUMENT and "null" in msg
    # not finished: uploaded only, then launched only
    b = h2v.Batch(ctx, 8, 8)
    refused(b, BAD_ARGUMENT, "finished")
    b.set_groups(2)
    flat, inst = b"".join(P[:8]), b"".join(v for i in I[:8] for col in i for v in col)
    b.upload(flat, len(P[0]), inst, [8], _rand_bytes(rand))
    refused(b, BAD_ARGUMENT, "finished")
    b.launch(with_pairing=False)
    refused(b, BAD_ARGUMENT, "finished")
    # a fold since the launch
    rec = torch.zeros(2 * ACC_BYTES, dtype=torch.uint8, device="cuda:0")
    b.export_accumulators(rec.data_ptr())
    b.fold_check_enqueue(rec.data_ptr(), 1)
    fin_b = b.finish_groups()
    assert fin_b[0] == [True, True]
    refused(b, BAD_ARGUMENT, "fold", fin_b)
    # a shard: a tail of draws longer than the upload
    b.set_groups(1)
    b.upload(flat, len(P[0]), inst, [8], _rand_bytes(rand + _draws(4, 11)))
    b.launch(with_pairing=False)
    fin_b = b.finish_groups()
    refused(b, BAD_ARGUMENT, "shard", fin_b)
    b.close()
    # a batch over other params
    other = circuits.setup_vector_mul(8, 8, s_seed=43)
    Po, Io = circuits.prove_vector_mul_batch(other, 2, seed=5, threads=2)
    co = _ctx(other)
    bo, fin_o = _stage(co, Po, Io, rand[:2], [1, 1])
    assert fin_o[0] == [True, True]
    refused(bo, BAD_ARGUMENT, "params", fin_o)
    bo.close(); co.close(); other.free()
    # a batch on another device
    if h2v.device_count() >= 2:
        c1 = _ctx(s, device=1)
        b1, fin_1 = _stage(c1, P[:8], I[:8], rand, [4, 4], equal=True)
        refused(b1, BAD_ARGUMENT, "device", fin_1)
        b1.close(); c1.close()
    # a journal one entry short of G: 2 entries in use, 4 free, a batch of 5 groups
    five, fin_5 = _stage(ctx, P[:8], I[:8], rand, [1, 2, 1, 3, 1])
    refused(five, UNSUPPORTED, "journal", fin_5)
    five.close()
    # the Python mirror's own refusals
    with pytest.raises(TypeError):
        acc.process_batch(ctx)
    keeper = h2v.Accumulator(ctx, journal=8, keep_inputs=True)
    with pytest.raises(ValueError, match="Batch.identify"):
        keeper.process_batch(good)
    assert keeper.read() == (ZERO, ZERO, 0, 0)
    keeper.close()
    # and the accumulator still works: four groups fill the journal exactly
    assert acc.process_batch(good) == (8, 0)
    exp = batch_reference.expected([(s, p, i) for p, i in zip(P[8:10] + P[:8], I[8:10] + I[:8])], _draws(2, 10) + rand)
    assert acc.finalize() == (True, exp[2], exp[3]) and len(acc.check_legs()) == 6
    assert good.finish_groups() == fin
    # the batch is uploaded again right after a feed, and a full journal refuses the next one
    good, fin = _stage(ctx, P[10:12], I[10:12], rand[:2], [2], batch=good)
    assert fin[0] == [True]
    before = (acc.read(), acc.check_legs())
    refused(good, UNSUPPORTED, "journal", fin)
    acc.close(); good.close()
