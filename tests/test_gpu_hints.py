"""Point hints through the C ABI and Batch (include/h2v_hints.h; halo2_verifier_amd/hints.py).

The invariant under test: the results of a launch depend on the uploaded proofs, instances and draws only; the hints, whatever bytes
they hold, change its time and nothing else.  Every case compares a hinted launch bit for bit with the launch of the same upload
without hints (and with the CPU oracle), and Batch.hint_stats() with the count tests/hints_reference.py gives: right hints,
adversarial hints, bad proofs under right-looking hints, the hints' lifetime, their export, the device forms, the other launch shapes
and consumers, and two host threads.  Proofs are the k = 8 circuits of tests/circuits.py."""
import ctypes
import random
import threading

import pytest

import circuits
import hints_reference as hr
from circuits import R_MOD

pytestmark = pytest.mark.gpu

N = 67
BAD = -16


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript, circuit_instances=s.circuit_instances)


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


def _rand_bytes(rand):
    return b"".join(r.to_bytes(32, "little") for r in rand)


def _flat(P, I):
    return b"".join(P), b"".join(b"".join(col) for i in I for col in i)


def _batch(ctx, n, groups=1, sizes=None, values=64):
    import halo2_verifier_amd as h2v
    b = h2v.Batch(ctx, max(n, 1), values)
    if sizes is not None:
        b.set_group_sizes(sizes)
    elif groups != 1:
        b.set_groups(groups)
    return b


def _upload(b, P, I, rand):
    flat, inst = _flat(P, I)
    b.upload(flat, len(P[0]), inst, [len(col) for col in I[0]], _rand_bytes(rand))


def _run(ctx, P, I, rand, hints=None, groups=1, sizes=None, pairing=True, keep=False):
    """upload, hints (None: none), launch, finish_groups -> (results, hint_stats) [, the batch]"""
    b = _batch(ctx, len(P), groups, sizes)
    _upload(b, P, I, rand)
    if hints is not None:
        b.set_hints(hints)
    b.launch(with_pairing=pairing)
    out = b.finish_groups(), b.hint_stats()
    if keep:
        return out + (b,)
    b.close()
    return out


def _points(offsets, P):
    return [pt for proof in P for pt in hr.points_of(offsets, proof)]


@pytest.fixture(scope="module")
def pool():
    from halo2_verifier_amd import hints
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, N, seed=4711, threads=16)
    c = _ctx(s)
    off = hints.point_offsets(c)
    rand = _draws(N, 99)
    yield dict(s=s, P=P, I=I, ctx=c, off=off, np=len(off), rand=rand, plain=_run(c, P, I, rand))
    c.close()
    s.free()


def test_point_offsets_are_the_plans(pool):
    from halo2_verifier_amd import hints
    shape = pool["ctx"].proof_shape()
    off = pool["off"]
    assert len(off) == shape["n_points"] > 0 and off == sorted(off) and len(set(off)) == len(off)
    assert all(o % 32 == 0 and o + 32 <= shape["proof_len"] for o in off)
    lib, n = hints._library(), ctypes.c_size_t(0)
    small = (ctypes.c_size_t * 1)()
    assert lib.h2v_hints_point_offsets(pool["ctx"]._h, small, 1, ctypes.byref(n)) == BAD and n.value == len(off)   # cap < Np; the count is written
    # every point of a valid proof decodes, and the library's rows are the reference's
    assert hints.for_proofs(off, b"".join(pool["P"][:3]), len(pool["P"][0])) == hr.rows(off, pool["P"][:3])
    assert all(hr.decode(pt) is not None for pt in _points(off, pool["P"][:3]))


# ------------------------------------------------------------------ 1. right hints
@pytest.mark.parametrize("n", [1, 5, 64, 67])
def test_right_hints_change_nothing(pool, n):
    from halo2_verifier_amd import hints
    P, I, rand, c = pool["P"][:n], pool["I"][:n], pool["rand"][:n], pool["ctx"]
    plain, plain_stats = _run(c, P, I, rand)
    got, stats = _run(c, P, I, rand, hints.for_proofs(pool["off"], b"".join(P), len(P[0])))
    assert got == plain
    ok, st, left, right = circuits.oracle_verify_batch(pool["s"], P, I, rand)
    assert got == ([ok], st, [left], [right]) and ok
    total = n * pool["np"]
    assert stats == (total, total, 0) and plain_stats == (total, 0, 0)


# ------------------------------------------------------------------ 2. any hints
@pytest.mark.parametrize("kind", hr.HINT_SETS)
def test_any_hints_change_nothing(pool, kind):
    pts = _points(pool["off"], pool["P"])
    h = hr.hint_set(kind, pts, seed=17)
    got, stats = _run(pool["ctx"], pool["P"], pool["I"], pool["rand"], h)
    assert got == pool["plain"][0]
    total = N * pool["np"]
    assert stats == (total, total, hr.count_misses(pts, h))
    if kind in ("zero", "other_root", "plus_p"):
        assert stats[2] == total
    if kind == "lane0_wrong":
        assert stats[2] == (total + 63) // 64          # exactly one per wave
    if kind == "right":
        assert stats[2] == 0


# ------------------------------------------------------------------ 3. bad proofs under right-looking hints
def _spoil(proof, off, how):
    b = bytearray(proof)
    if how == "sign":
        b[off + 31] ^= 0x40
    elif how == "nonresidue":
        b[off:off + 32] = hr.encode(hr.non_residue_x(12345), b[off + 31] & 0x40)
    elif how == "x_ge_p":
        b[off:off + 32] = hr.encode(hr.P + 5, 0)
    else:
        b[off + 31] |= 0x80
    return bytes(b)


@pytest.mark.parametrize("slot", ["main", "opening"])
@pytest.mark.parametrize("how", ["sign", "nonresidue", "x_ge_p", "identity"])
def test_a_bad_proof_under_the_original_hints(pool, how, slot):
    """proof 41 of the 67 carries a spoiled point; the hints are the ORIGINAL proofs' (for the flipped sign: the y of P where the proof
    now says -P): the launch decodes what the bytes say, as the launch without hints and the oracle do"""
    from halo2_verifier_amd import hints
    c, I, rand = pool["ctx"], pool["I"], pool["rand"]
    off = pool["off"][0] if slot == "main" else pool["off"][-1]
    P = list(pool["P"])
    P[41] = _spoil(P[41], off, how)
    original = hints.for_proofs(pool["off"], b"".join(pool["P"]), len(P[0]))
    plain, _ = _run(c, P, I, rand)
    got, stats = _run(c, P, I, rand, original)
    assert got == plain
    ok, st, left, right = circuits.oracle_verify_batch(pool["s"], P, I, rand)
    assert got == ([ok], st, [left], [right]) and not ok
    assert stats == (N * pool["np"], N * pool["np"], 1)            # the one point whose hint is not its y (or that has none)
    assert [v for i, v in enumerate(got[1]) if i != 41] == [0] * (N - 1)      # the other proofs' statuses are untouched
    if how == "sign":
        assert got[1][41] == 0                                # it decodes, to -P: only the pairing rejects the batch
        assert hr.decode(P[41][off:off + 32]) == hr.P - hr.decode(pool["P"][41][off:off + 32])
    else:
        assert got[1][41] == (-5 if slot == "main" else -4)   # H2V_ERR_TRANSCRIPT / H2V_ERR_OPENING
        assert c.verify_each(P[40:43], I[40:43]) == got[1][40:43]


# ------------------------------------------------------------------ 4. lifetime
def test_the_hints_live_as_long_as_their_upload(pool):
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import hints
    c, P, I, rand = pool["ctx"], pool["P"], pool["I"], pool["rand"]
    right = hints.for_proofs(pool["off"], b"".join(P), len(P[0]))
    total = N * pool["np"]
    lib = hints._library()
    b = _batch(c, N)
    refuse = lambda n=N, y=right: lib.h2v_batch_set_hints(b._h, n, y)
    assert refuse() == BAD and "h2v_batch_set_hints" in h2v._lib.last_error()      # before any upload
    _upload(b, P, I, rand)
    assert refuse(N - 1) == BAD and refuse(N + 1) == BAD                             # n != the upload's
    b.set_hints(right)
    b.launch()
    assert (b.finish_groups(), b.hint_stats()) == (pool["plain"][0], (total, total, 0))
    assert refuse() == BAD                                                           # after a launch
    with pytest.raises(h2v.H2VError):
        b.set_hints(None)
    b.launch()                                                                       # a relaunch of the hinted upload: the refusals left it launchable
    assert (b.finish_groups(), b.hint_stats()) == (pool["plain"][0], (total, total, 0))
    _upload(b, P, I, rand)                                                           # a new upload drops the hints
    b.launch()
    assert (b.finish_groups(), b.hint_stats()) == (pool["plain"][0], (total, 0, 0))
    _upload(b, P, I, rand)
    b.set_hints(hr.hint_set("zero", _points(pool["off"], P)))
    b.set_hints(None)                                                                # dropped again: an unhinted launch
    b.launch()
    assert (b.finish_groups(), b.hint_stats()) == (pool["plain"][0], (total, 0, 0))
    flat, inst = _flat(P, I)
    b.upload_launch(flat, len(P[0]), inst, [8], _rand_bytes(rand))
    assert refuse() == BAD                                                           # after upload_launch
    assert (b.finish_groups(), b.hint_stats()) == (pool["plain"][0], (total, 0, 0))
    b.close()


# ------------------------------------------------------------------ 5. export
def test_a_launch_leaves_the_hints_for_the_next_verifier(pool):
    import halo2_verifier_amd as h2v
    c, I, rand, off = pool["ctx"], pool["I"], pool["rand"], pool["off"]
    P = list(pool["P"])
    P[3] = _spoil(P[3], off[1], "nonresidue")
    P[66] = _spoil(_spoil(P[66], off[-1], "x_ge_p"), off[0], "identity")
    plain, stats, b = _run(c, P, I, rand, keep=True)
    assert stats == (N * pool["np"], 0, 0) and plain[1][3] == -5 and plain[1][66] == -5
    left = b.hints()
    assert left == hr.rows(off, P) and left.count(bytes(32)) >= 3
    row = 32 * pool["np"]
    assert b.hints(5, 7) == left[5 * row:12 * row] and b.hints(66) == left[66 * row:] and b.hints(67) == b"" and b.hints(0, 0) == b""
    lib = h2v.hints._library()
    buf = ctypes.create_string_buffer(row * 4)
    for first, count in ((68, 0), (64, 4), (0, 68)):
        assert lib.h2v_batch_hints(b._h, first, count, buf) == BAD and "outside the upload" in h2v._lib.last_error()
    assert lib.h2v_batch_hints(b._h, 0, 1, None) == BAD
    # fed back: every decodable point hits, the three others miss
    got, stats2 = _run(c, P, I, rand, left)
    assert got == plain and stats2 == (N * pool["np"], N * pool["np"], 3)
    # and the hinted launch leaves the same rows
    b.close()
    (res3, _, b3) = _run(c, P, I, rand, hr.hint_set("random", _points(off, P), seed=3), keep=True)
    assert res3 == plain and b3.hints() == left
    b3.close()
    unlaunched = _batch(c, N)
    _upload(unlaunched, P, I, rand)
    assert lib.h2v_batch_hints(unlaunched._h, 0, 1, buf) == BAD and lib.h2v_batch_hint_stats(unlaunched._h, None, None, None) == BAD
    unlaunched.close()


# ------------------------------------------------------------------ 6. device forms
def test_hints_from_and_into_device_memory(pool):
    import torch
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import hints
    c, P, I, rand, npts = pool["ctx"], pool["P"], pool["I"], pool["rand"], pool["np"]
    row = 32 * npts
    right = hints.for_proofs(pool["off"], b"".join(P), len(P[0]))
    flat, inst = _flat(P, I)
    dev = lambda raw, cols: torch.frombuffer(bytearray(raw), dtype=torch.uint8).reshape(len(raw) // cols, cols).cuda()
    padded = torch.full((N, row + 16), 0xAB, dtype=torch.uint8)
    padded[:, :row] = torch.frombuffer(bytearray(right), dtype=torch.uint8).reshape(N, row)
    padded = padded.cuda()
    b = _batch(c, N)
    b.upload_tensors(dev(flat, len(P[0])), dev(inst, 8 * 32), [8], dev(_rand_bytes(rand), 32))
    b.set_hints_tensor(padded[:, :row])
    b.launch()
    status = torch.empty(N, dtype=torch.int32, device="cuda:0")
    ok = torch.empty(1, dtype=torch.int32, device="cuda:0")
    lx, rx = torch.empty((1, 64), dtype=torch.uint8, device="cuda:0"), torch.empty((1, 64), dtype=torch.uint8, device="cuda:0")
    b.finish_into(status=status, group_ok=ok, left_xy=lx, right_xy=rx)
    out = torch.full((N, row + 32), 0xCD, dtype=torch.uint8, device="cuda:0")
    b.hints_into(out[:, :row])
    part = torch.full((9, row), 0xCD, dtype=torch.uint8, device="cuda:0")
    b.hints_into(part, 50, 9)
    torch.cuda.synchronize()
    plain = pool["plain"][0]
    assert ([bool(ok.item())], status.tolist(), [bytes(lx.cpu().numpy().tobytes())], [bytes(rx.cpu().numpy().tobytes())]) == plain
    assert b.hint_stats() == (N * npts, N * npts, 0)
    host = out.cpu()
    assert host[:, :row].numpy().tobytes() == b.hints() == right and bool((host[:, row:] == 0xCD).all())     # the padding is not touched
    assert part.cpu().numpy().tobytes() == right[50 * row:59 * row]
    assert b.finish_groups() == plain
    # refusals, before any device work: the batch stays launchable
    _upload(b, P, I, rand)
    lib = hints._library()
    vp = ctypes.c_void_p
    host_buf = ctypes.create_string_buffer(N * row + 16)
    addr = (ctypes.addressof(host_buf) + 15) & ~15
    assert lib.h2v_batch_set_hints_device(b._h, N, vp(addr), row) == BAD and "not device memory" in h2v._lib.last_error()
    assert lib.h2v_batch_set_hints_device(b._h, N, vp(padded.data_ptr() + 8), row + 16) == BAD and "16-byte aligned" in h2v._lib.last_error()
    assert lib.h2v_batch_set_hints_device(b._h, N, vp(padded.data_ptr()), row + 8) == BAD and "row_stride" in h2v._lib.last_error()
    assert lib.h2v_batch_set_hints_device(b._h, N, vp(padded.data_ptr()), row - 16) == BAD
    # an allocation too short by one row: torch hands out pieces of larger segments, so the rows are made to end one row behind the segment's end
    seg = next(x for x in torch.cuda.memory_snapshot() if x["address"] <= padded.data_ptr() < x["address"] + x["total_size"])
    short = seg["address"] + seg["total_size"] - (N - 1) * row
    assert lib.h2v_batch_set_hints_device(b._h, N, vp(short), row) == BAD and "allocation" in h2v._lib.last_error()
    assert lib.h2v_batch_set_hints_device(b._h, N - 1, vp(short), row) == BAD and "n is not the upload's" in h2v._lib.last_error()
    b.launch()
    assert b.finish_groups() == plain and b.hint_stats() == (N * npts, 0, 0)
    assert lib.h2v_batch_hints_device(b._h, 0, N, vp(short), row) == BAD and "allocation" in h2v._lib.last_error()
    assert lib.h2v_batch_hints_device(b._h, 0, N, vp(addr), row) == BAD
    assert lib.h2v_batch_hints_device(b._h, 1, N, vp(padded.data_ptr()), row + 16) == BAD and "outside the upload" in h2v._lib.last_error()
    assert b.finish_groups() == plain
    b.close()


# ------------------------------------------------------------------ 7. other launch shapes and consumers
def _right(pool, P):
    from halo2_verifier_amd import hints
    return hints.for_proofs(pool["off"], b"".join(P), len(P[0]))


def test_equal_groups(pool):
    P, I, rand = pool["P"][:64], pool["I"][:64], pool["rand"][:64]
    plain, _ = _run(pool["ctx"], P, I, rand, groups=4)
    got, stats = _run(pool["ctx"], P, I, rand, _right(pool, P), groups=4)
    assert got == plain and all(got[0]) and len(got[0]) == 4 and stats == (64 * pool["np"], 64 * pool["np"], 0)


def test_unequal_groups_with_a_proof_only_the_pairing_rejects(pool):
    P, I, rand = list(pool["P"]), pool["I"], pool["rand"]
    plen = len(P[0])
    chunk = max(o for o in range(0, plen - 32, 32) if o not in pool["off"])    # a scalar of the proof: an evaluation
    bad = bytearray(P[3]); bad[chunk] ^= 1; P[3] = bytes(bad)
    plain, _ = _run(pool["ctx"], P, I, rand, sizes=[1, 5, 61])
    got, stats = _run(pool["ctx"], P, I, rand, _right(pool, P), sizes=[1, 5, 61])
    assert got == plain and got[0] == [True, False, True] and not any(got[1]) and stats[2] == 0
    for g, (lo, hi) in enumerate(((0, 1), (1, 6), (6, 67))):
        ok, st, left, right = circuits.oracle_verify_batch(pool["s"], P[lo:hi], I[lo:hi], rand[lo:hi])
        assert (got[0][g], got[2][g], got[3][g]) == (ok, left, right)


def _exported(pool, h):
    """launch(with_pairing=False) + export_accumulators of 64 proofs in 4 groups under the hints h -> (record bytes, statuses + channels)"""
    import torch
    from halo2_verifier_amd.distributed import ACC_BYTES
    P, I, rand = pool["P"][:64], pool["I"][:64], pool["rand"][:64]
    b = _batch(pool["ctx"], 64, groups=4)
    _upload(b, P, I, rand)
    if h is not None:
        b.set_hints(h)
    b.launch(with_pairing=False)
    dst = torch.zeros(4 * ACC_BYTES, dtype=torch.uint8, device="cuda:0")
    b.export_accumulators(dst.data_ptr())
    res = b.finish_groups()
    torch.cuda.synchronize()
    b.close()
    return dst.cpu().numpy().tobytes(), res[1:]


R_INV = pow(1 << 261, -1, hr.P)      # the limbs hold value * 2^261 mod p (nine limbs of 29 bits)


def _record_points(raw):
    """records -> per record its four header words and its 2 x parts pieces as canonical affine points (None: the identity).  A piece is
    a Jacobian (X, Y, Z) in 9 limbs of 29 bits per coordinate, of whatever representative below 2p the arithmetic left."""
    import numpy as np
    w = np.frombuffer(raw, dtype="<u4").tolist()
    assert len(w) % 328 == 0
    out = []
    for r in range(0, len(w), 328):
        head, pts = w[r:r + 4], []
        assert 1 <= head[1] <= 6
        for side in range(2):
            for j in range(head[1]):
                k = r + 4 + 27 * (6 * side + j)
                X, Y, Z = [sum(v << (29 * i) for i, v in enumerate(w[k + 9 * q:k + 9 * q + 9])) * R_INV % hr.P for q in range(3)]
                pts.append(None if Z == 0 else (X * pow(Z, -2, hr.P) % hr.P, Y * pow(Z, -3, hr.P) % hr.P))
        out.append((head, pts))
    return out


def test_exported_accumulators_are_the_same_records(pool):
    """launch(with_pairing=False) + export_accumulators with right hints and with hints on even points only: the records of the
    launch without hints — the header words, and every piece as a point.

    Not byte for byte, which no two launches of one upload are, hints or none: the pieces are Jacobian coordinates whose
    representation follows the order in which the MSM's additions happen to run.  Measured on an MI355X, 64 proofs in 4 groups
    (5248 bytes of records): two launches WITHOUT hints differ in 2075 bytes, a launch without and one with right hints in 2072, two
    launches with the same hints in 2085 — and every piece is the same affine point in all of them.  So the comparison is made where a
    record is defined: on the points; the repeated unhinted launch is held to the same, so that a pass means what it says."""
    P = pool["P"][:64]
    plain, again = _exported(pool, None), _exported(pool, None)
    right = _exported(pool, _right(pool, P))
    even = _exported(pool, hr.hint_set("even_lanes", _points(pool["off"], P)))
    assert plain[1] == again[1] == right[1] == even[1]
    want = _record_points(plain[0])
    assert len(want) == 4 and any(pt is not None for _, pts in want for pt in pts)
    assert _record_points(again[0]) == want and _record_points(right[0]) == want and _record_points(even[0]) == want
    print("bytes of the %d-byte records that differ from the first unhinted launch's: unhinted again %d, right hints %d, even lanes %d"
          % ((len(plain[0]),) + tuple(sum(1 for x, y in zip(plain[0], o[0]) if x != y) for o in (again, right, even))))


@pytest.mark.parametrize("multiopen,transcript", [(circuits.GWC, circuits.BLAKE2B), (circuits.SHPLONK, circuits.KECCAK256)], ids=["gwc", "keccak"])
def test_other_plans(multiopen, transcript):
    from halo2_verifier_amd import hints
    s = circuits.setup_wide(8).set_options(multiopen, transcript)
    proofs = [circuits.prove_wide(s, witness_seed=3 + i, rng_seed=13 + i) for i in range(3)]
    P, I = [p for p, _ in proofs], [i for _, i in proofs]
    c = _ctx(s)
    rand = _draws(3, 7)
    off = hints.point_offsets(c)
    plain, _ = _run(c, P, I, rand)
    got, stats = _run(c, P, I, rand, hints.for_proofs(off, b"".join(P), len(P[0])))
    ok, st, left, right = circuits.oracle_verify_batch(s, P, I, rand)
    assert got == plain == ([ok], st, [left], [right]) and ok and stats == (3 * len(off), 3 * len(off), 0)
    c.close(); s.free()


def test_two_circuit_instances_byte_order_is_slot_order():
    """one transcript over two circuit instances: the j-th hint of a row belongs to the j-th point in BYTE order, which is the order
    of the kernel's point slots — hints made from the sorted offsets all hit"""
    from halo2_verifier_amd import hints
    s = circuits.setup_vector_mul(8, 8).set_circuit_instances(2)
    proofs = [circuits.prove_vector_mul_multi(s, 2, seed=10 + i, rng_seed=11 + i) for i in range(5)]
    P, I = [p for p, _ in proofs], [i for _, i in proofs]
    c = _ctx(s)
    off = hints.point_offsets(c)
    assert off == sorted(off) and len(off) == c.proof_shape()["n_points"]
    rand = _draws(5, 8)
    plain, _ = _run(c, P, I, rand)
    got, stats = _run(c, P, I, rand, hr.rows(sorted(off), P))
    ok, st, left, right = circuits.oracle_verify_batch(s, P, I, rand)
    assert got == plain == ([ok], st, [left], [right]) and ok and stats == (5 * len(off), 5 * len(off), 0)
    c.close(); s.free()


def test_the_consumers_of_a_launch_see_no_difference(pool):
    import halo2_verifier_amd as h2v
    P, I, rand = list(pool["P"]), pool["I"], pool["rand"]
    plen = len(P[0])
    chunk = max(o for o in range(0, plen - 32, 32) if o not in pool["off"])
    bad = bytearray(P[30]); bad[chunk] ^= 1; P[30] = bytes(bad)               # only the pairing rejects it
    P[50] = _spoil(P[50], pool["off"][0], "x_ge_p")
    seen = []
    for h in (None, _right(pool, P), hr.hint_set("lane0_wrong", _points(pool["off"], P))):
        res, stats, b = _run(pool["ctx"], P, I, rand, h, keep=True)
        acc = h2v.Accumulator(pool["ctx"])
        seen.append((res, b.recheck([(0, 30), (30, 1), (31, 19), (51, 16)]), b.identify()[:2], b.guards(29, 3), b.guards(50, 1), acc.process_batch(b), acc.read()))
        acc.close(); b.close()
    assert seen[0] == seen[1] == seen[2]
    assert seen[0][0][0] == [False] and seen[0][2][0][30] == -2 and seen[0][2][0][50] == -5 and seen[0][1][0] == [True, False, True, True]


# ------------------------------------------------------------------ 8. two host threads
def test_two_threads_one_hinted_one_not(pool):
    c, P, I = pool["ctx"], pool["P"], pool["I"]
    rands = [_draws(N, 1), _draws(N, 2)]
    hints_of = [_right(pool, P), None]
    want = [_run(c, P, I, rands[k], hints_of[k]) for k in range(2)]
    got, errors = [None, None], []

    def work(k):
        try:
            for _ in range(3):
                got[k] = _run(c, P, I, rands[k], hints_of[k])
                assert got[k] == want[k]
        except BaseException as e:     # noqa: BLE001
            errors.append(e)
    threads = [threading.Thread(target=work, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    assert got == want and want[0][0] != want[1][0] and want[0][1][1] == N * pool["np"] and want[1][1][1] == 0
