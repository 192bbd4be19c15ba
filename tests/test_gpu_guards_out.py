"""Every proof's Guard out of a launch, through the C ABI (include/h2v_guards.h; Batch.guard_shape / guards / guards_into /
guards_append): the host form against the definition in Python integers (tests/guards_out_reference.py: the CPU oracle's Guard of
each proof times the group's suffix-product multipliers), exactly — SHPLONK as the sequence, GWC as the merged sequence and per proof
as {base: sum of scalars}; mult and status too.  The device form equals the host form bit for bit between intact guard bands and
returns under a busy stream; the append form fills resident MSM objects whose checks are finish_groups' verdicts and accumulators;
the calls change nothing a finish reports; the refusals come before any device work.

Also: a launch without a pairing (the accumulators still in pieces), a smaller upload into a larger batch behind another launch, the
2^24-term limit on an object filled on the device to one term below it, and a draw >= r uploaded from device memory.

Not provoked here: a guard-variant upload.  Only h2v_guard_msm's scratch batch is one, and no public call hands it out
(tests/test_gpu_accumulator_batch.py leaves the same refusal of h2v_accumulator_process_batch out for the same reason)."""
import ctypes
import random
import time

import pytest

import circuits
import guards_out_reference as gr
from circuits import R_MOD

pytestmark = pytest.mark.gpu

ZERO = bytes(64)
BAND = 64
TR = 18      # the right channel of the toy VK (setup_vector_mul): 18 terms per proof; its left channel (SHPLONK) has one


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript)


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 15, seed=8642, threads=15)
    c = _ctx(s)
    yield s, P, I, c
    c.close()
    s.free()


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


def _launched(ctx, P, I, rand, sizes, pairing=True):
    import halo2_verifier_amd as h2v
    col_lens = [len(col) for col in I[0]]
    b = h2v.Batch(ctx, len(P), sum(col_lens))
    if len(set(sizes)) == 1:
        b.set_groups(len(sizes))
    else:
        b.set_group_sizes(sizes)
    b.upload(b"".join(P), len(P[0]), b"".join(v for inst in I for col in inst for v in col), col_lens, b"".join(r.to_bytes(32, "little") for r in rand))
    b.launch(with_pairing=pairing)
    return b


def _ints(row):
    n = lambda xs: [int.from_bytes(x, "little") for x in xs]
    return dict(left_scalars=n(row["left_scalars"]), left_bases=list(row["left_bases"]), right_scalars=n(row["right_scalars"]),
                right_bases=list(row["right_bases"]), mult=int.from_bytes(row["mult"], "little"), status=row["status"])


def _compare(s, got, exp, P=None, I=None):
    """got: Batch.guards' rows; exp: guards_out_reference.expected's.  Every field exactly; GWC also per proof as {base: sum}"""
    assert len(got) == len(exp)
    for j, (g, e) in enumerate(zip(got, exp)):
        assert _ints(g) == e, j
        if s.multiopen == circuits.GWC and e["status"] == 0 and P is not None:
            rc, raw = circuits.oracle_guard(s, P[j], I[j])
            per_query = [int.from_bytes(x, "little") * e["mult"] % R_MOD for x in raw["right_scalars"]]
            assert len(per_query) > len(e["right_scalars"])
            assert gr.by_base(_ints(g)["right_scalars"], g["right_bases"]) == gr.by_base(per_query, raw["right_bases"]), j


def test_one_proof(pool):
    s, P, I, ctx = pool
    rand = _draws(1, 1)
    b = _launched(ctx, P[:1], I[:1], rand, [1])
    assert b.guard_shape() == (1, TR)
    _compare(s, b.guards(), gr.expected(s, P[:1], I[:1], rand, [1]))
    b.close()


@pytest.mark.parametrize("n", [14, 15])
def test_unit_draws_are_the_raw_guards_of_guard_msm(pool, n):
    """with unit draws every row is Context.guard_msm of its proof.  n = 14 is the issue's case; this VK's T_R is 18, not 19, so 14
    proofs are 252 right terms, one workgroup, and n = 15 (270 terms) is the case that runs more than one"""
    s, P, I, ctx = pool
    P, I = P[:n], I[:n]
    b = _launched(ctx, P, I, [1] * n, [n])
    got = b.guards()
    assert (n * TR > 256) == (n == 15)
    _compare(s, got, gr.expected(s, P, I, [1] * n, [n]))
    for j in range(n):
        rc, g = ctx.guard_msm(P[j], I[j])
        assert rc == 0
        for k in ("left_scalars", "left_bases", "right_scalars", "right_bases"):
            assert got[j][k] == g[k], (j, k)
        assert got[j]["mult"] == (1).to_bytes(32, "little") and got[j]["status"] == 0
    b.close()


def test_equal_groups_ranges_and_independence(pool):
    """n = 12 in 3 equal groups, random draws; a sub-range that crosses a group boundary; the call before and after the host finish,
    twice, gives the same, and the finish gives what it gives without the call (a second batch that never made it)"""
    s, P, I, ctx = pool
    n, sizes = 12, [4, 4, 4]
    rand = _draws(n, 3)
    exp = gr.expected(s, P[:n], I[:n], rand, sizes)
    b = _launched(ctx, P[:n], I[:n], rand, sizes)
    before = b.guards()
    _compare(s, before, exp)
    _compare(s, b.guards(3, 6), exp[3:9])
    _compare(s, b.guards(11), exp[11:])
    assert b.guards(5, 0) == [] and b.guards(12) == []
    want = b.finish_groups()
    assert b.guards() == before and b.guards() == before
    assert b.finish_groups() == want and want[0] == [True] * 3
    plain = _launched(ctx, P[:n], I[:n], rand, sizes)
    assert plain.finish_groups() == want
    assert b.recheck([(0, 4), (5, 2)]) == plain.recheck([(0, 4), (5, 2)])
    assert b.identify() == plain.identify()
    b.launch()                                                # a relaunch of the same upload: the same Guards
    assert b.guards() == before and b.finish_groups() == want
    b.close(); plain.close()


def test_unequal_groups_with_a_zero_draw(pool):
    s, P, I, ctx = pool
    sizes = [1, 5, 2]
    rand = _draws(8, 4)
    rand[3] = 0                                               # inside the middle group: proofs 1 and 2 have a zero multiplier
    exp = gr.expected(s, P[:8], I[:8], rand, sizes)
    assert [e["mult"] for e in exp[:4]] == [1, 0, 0, exp[3]["mult"]] and exp[3]["mult"] != 0
    b = _launched(ctx, P[:8], I[:8], rand, sizes)
    got = b.guards()
    _compare(s, got, exp)
    assert not any(_ints(got[1])["right_scalars"]) and got[1]["right_bases"] == exp[1]["right_bases"] != [ZERO] * TR
    b.close()


def test_failing_proofs_are_zero_rows(pool):
    """a broken point and a non-canonical scalar in the middle of a group: zero rows, their statuses, the neighbours untouched"""
    s, P, I, ctx = pool
    n, sizes = 12, [6, 6]
    P2 = list(P[:n])
    x = bytearray(P2[2]); x[32:64] = b"\xff" * 32; P2[2] = bytes(x)                  # a point that does not decode
    P2[8] = P2[8][:-96] + b"\xff" * 32 + P2[8][-64:]                                 # a scalar >= r
    rand = _draws(n, 5)
    exp = gr.expected(s, P2, I[:n], rand, sizes)
    clean = gr.expected(s, P[:n], I[:n], rand, sizes)
    b = _launched(ctx, P2, I[:n], rand, sizes)
    got = b.guards()
    _compare(s, got, exp)
    assert [g["status"] for g in got] == [0, 0, exp[2]["status"], 0, 0, 0, 0, 0, -5, 0, 0, 0] and exp[2]["status"] != 0
    for j in (2, 8):
        assert set(got[j]["right_bases"]) == {ZERO} and set(got[j]["left_bases"]) == {ZERO}
        assert set(got[j]["right_scalars"]) | set(got[j]["left_scalars"]) == {bytes(32)}
    for j in (1, 3, 7, 9):
        assert _ints(got[j]) == clean[j]
    want = b.finish_groups()
    assert want[1] == [g["status"] for g in got]
    b.close()


@pytest.mark.parametrize("multiopen,transcript", [(circuits.GWC, circuits.BLAKE2B), (circuits.SHPLONK, circuits.KECCAK256)], ids=["gwc", "keccak"])
def test_other_plans(multiopen, transcript):
    import halo2_verifier_amd as h2v
    s = circuits.setup_vector_mul(8, 4).set_options(multiopen, transcript)
    P, I = circuits.prove_vector_mul_batch(s, 6, seed=77 + multiopen, threads=6)
    c = _ctx(s)
    sizes = [2, 4]
    rand = _draws(6, 6)
    P2 = list(P); P2[4] = P2[4][:-96] + b"\xff" * 32 + P2[4][-64:]
    b = _launched(c, P2, I, rand, sizes)
    exp = gr.expected(s, P2, I, rand, sizes)
    got = b.guards()
    _compare(s, got, exp, P2, I)
    assert got[4]["status"] != 0 and b.guard_shape() == (len(exp[0]["left_scalars"]), len(exp[0]["right_scalars"]))
    if multiopen == circuits.GWC:
        assert b.guard_shape()[0] > 1                        # several witness points: the left channel is not strided
        rc, g = c.guard_msm(P[0], I[0])
        assert rc == 0 and len(g["right_scalars"]) > b.guard_shape()[1]   # h2v_guard_msm keeps the per-query list
    with pytest.raises(h2v.H2VError, match="outside the upload"):
        b._lib.h2v_batch_guards.restype = ctypes.c_int
        h2v._lib.check(b._lib.h2v_batch_guards(b._h, ctypes.c_size_t(3), ctypes.c_size_t(4), None, None, None, None, None, None))
    b.close(); c.close(); s.free()


def test_wide_vk_with_lookups_and_shuffle():
    s = circuits.setup_wide(8)
    proofs = [circuits.prove_wide(s, witness_seed=3 + i, rng_seed=13 + i) for i in range(3)]
    P, I = [p for p, _ in proofs], [i for _, i in proofs]
    c = _ctx(s)
    rand = _draws(3, 7)
    b = _launched(c, P, I, rand, [1, 2])
    _compare(s, b.guards(), gr.expected(s, P, I, rand, [1, 2]))
    b.close(); c.close(); s.free()


# ---- the device form

def _banded(torch, size, dtype):
    """`size` elements and a band behind them, every byte 0xEE -> (the whole tensor, the view the call is given)"""
    whole = torch.full((size + BAND,), 0xEE if dtype == torch.uint8 else -286331154, dtype=dtype, device="cuda:0")
    return whole, whole[:size]


def _device_outputs(b, count):
    import torch
    from halo2_verifier_amd import guards
    sizes = guards.output_sizes(count, b.guard_shape())
    out = {}
    for what, size in zip(guards.OUTPUTS, sizes):
        out[what] = _banded(torch, size // 4, torch.int32) if what == "status" else _banded(torch, size, torch.uint8)
    torch.cuda.synchronize()                                # (the presets are in place before any other stream writes)
    return out


def _host_bytes(rows):
    cat = lambda k: b"".join(x for r in rows for x in r[k])
    return dict(left_scalars=cat("left_scalars"), left_bases=cat("left_bases"), right_scalars=cat("right_scalars"), right_bases=cat("right_bases"),
                mult=b"".join(r["mult"] for r in rows), status=[r["status"] for r in rows])


def _check_device(out, rows):
    import torch
    torch.cuda.synchronize()
    host = _host_bytes(rows)
    for what, (whole, view) in out.items():
        band = whole[view.numel():]
        if what == "status":
            assert view.tolist() == host[what] and set(band.tolist()) == {-286331154}, what
        else:
            assert bytes(view.cpu().numpy().tobytes()) == host[what], what
            assert set(band.tolist()) == {0xEE}, what


def test_device_form_equals_the_host_form(pool):
    s, P, I, ctx = pool
    n, sizes = 12, [4, 4, 4]
    P2 = list(P[:n]); P2[5] = P2[5][:-96] + b"\xff" * 32 + P2[5][-64:]
    rand = _draws(n, 8)
    b = _launched(ctx, P2, I[:n], rand, sizes)
    for first, count in ((0, n), (3, 6)):
        out = _device_outputs(b, count)
        b.guards_into(first, count, **{k: v[1] for k, v in out.items()})
        _check_device(out, b.guards(first, count))
    # one output at a time, and raw addresses
    out = _device_outputs(b, n)
    for k, (whole, view) in out.items():
        b.guards_into(0, n, **{k: view if k != "mult" else view.data_ptr()})
    _check_device(out, b.guards())
    want = b.finish_groups()
    plain = _launched(ctx, P2, I[:n], rand, sizes)
    assert plain.finish_groups() == want and want[1][5] == -5
    b.close(); plain.close()


def test_no_host_wait_behind_a_busy_stream(pool):
    """about a second of spinning is queued on the batch's stream behind a launch: guards_into returns while it still runs"""
    import torch
    s, P, I, ctx = pool
    n, sizes = 12, [4, 4, 4]
    rand = _draws(n, 9)
    b = _launched(ctx, P[:n], I[:n], rand, sizes)
    rows = b.guards()
    want = b.finish_groups()
    stream = torch.cuda.ExternalStream(b.stream, device="cuda:0")
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    with torch.cuda.stream(stream):                        # how long 10^7 of _sleep's cycles take here
        t0.record(); torch.cuda._sleep(10_000_000); t1.record()
    t1.synchronize()
    cycles = int(10_000_000 * 1000.0 / max(t0.elapsed_time(t1), 1e-3))
    out = _device_outputs(b, n)
    b.launch()
    behind = torch.cuda.Event()
    with torch.cuda.stream(stream):
        torch.cuda._sleep(cycles)
        behind.record()
    began = time.perf_counter()
    b.guards_into(0, n, **{k: v[1] for k, v in out.items()})
    took = time.perf_counter() - began
    assert not behind.query(), f"guards_into returned after {took:.3f} s, when the stream's earlier work was done"
    _check_device(out, rows)
    assert b.finish_groups() == want
    b.close()


# ---- the append form

def test_append_form(pool):
    """per group one (left, right) pair filled by guards_append of the group's range: the objects' terms are the host form's, and
    dual_check_many over the pairs gives finish_groups' verdicts and accumulators"""
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    sizes = [3, 6, 5]
    n = sum(sizes)
    I2 = list(I[:n])
    I2[4] = [[circuits.le32(5)] + I2[4][0][1:]]                # a wrong public input in group 1: only the pairing rejects it
    rand = _draws(n, 10)
    b = _launched(ctx, P[:n], I2, rand, sizes)
    rows = b.guards()
    duals, lo = [], 0
    for sz in sizes:
        d = h2v.DualMSM(ctx)
        assert b.guards_append(d.left, d.right, lo, sz) == 0
        assert len(d.left) == sz and len(d.right) == TR * sz
        host = _host_bytes(rows[lo:lo + sz])
        assert b"".join(x.to_bytes(32, "little") for x in d.right.scalars()) == host["right_scalars"] and b"".join(d.right.bases()) == host["right_bases"]
        assert b"".join(x.to_bytes(32, "little") for x in d.left.scalars()) == host["left_scalars"] and b"".join(d.left.bases()) == host["left_bases"]
        duals.append(d); lo += sz
    want = b.finish_groups()
    assert want[0] == [True, False, True] and want[1] == [0] * n
    ok, lefts, rights = h2v.dual_check_many(duals)
    assert (ok, lefts, rights) == (want[0], want[2], want[3])
    # behind terms an object already has, one channel at a time, and a failing proof counted
    m = h2v.MSMKZG(ctx)
    m.append_terms([7], [ZERO])
    assert b.guards_append(None, m, 1, 2) == 0 and len(m) == 1 + 2 * TR
    assert m.scalars()[0] == 7 and b"".join(x.to_bytes(32, "little") for x in m.scalars(1)) == _host_bytes(rows[1:3])["right_scalars"]
    assert b.guards_append(m, None, 13, 1) == 0 and len(m) == 2 + 2 * TR and m.bases(1 + 2 * TR) == rows[13]["left_bases"]
    # refusals leave length and read-back as they were
    before = (len(m), m.scalars(), m.bases())
    for call, match in ((lambda: b.guards_append(m, m, 0, 1), "same object"),
                        (lambda: h2v._lib.check(b._lib.h2v_batch_guards_append(b._h, ctypes.c_size_t(10), ctypes.c_size_t(5), m._handle(), None, None)), "outside the upload")):
        with pytest.raises((ValueError, h2v.H2VError), match=match):
            call()
    with pytest.raises(h2v.H2VError, match="same object"):
        h2v._lib.check(b._lib.h2v_batch_guards_append(b._h, ctypes.c_size_t(0), ctypes.c_size_t(1), m._handle(), m._handle(), None))
    other = circuits.setup_vector_mul(8, 8, s_seed=99)         # another SRS: an object over other params
    oc = _ctx(other)
    foreign = h2v.MSMKZG(oc)
    with pytest.raises(h2v.H2VError, match="other params"):
        b.guards_append(foreign, m, 0, 2)
    assert len(foreign) == 0 and (len(m), m.scalars(), m.bases()) == before
    assert b.finish_groups() == want
    foreign.close(); oc.close(); other.free()
    P3 = list(P[:n]); P3[1] = P3[1][:-96] + b"\xff" * 32 + P3[1][-64:]
    b2 = _launched(ctx, P3, I[:n], rand, sizes)
    d = h2v.DualMSM(ctx)
    assert b2.guards_append(d.left, d.right, 0, 3) == 1 and b2.guards_append(d.left, d.right, 3, 3) == 0
    assert d.right.scalars(TR, TR) == [0] * TR and d.right.bases(TR, TR) == [ZERO] * TR
    for x in duals + [d]:
        x.close()
    m.close(); b.close(); b2.close()


# ---- refusals

def test_lifecycle_refusals(pool):
    import numpy as np
    import torch
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    n = 8
    b = h2v.Batch(ctx, n, 8)
    for call in (lambda: b.guard_shape(), ):
        with pytest.raises(h2v.H2VError, match="nothing uploaded"):
            call()
    b.n = n                                                  # (what an upload would have set: the library itself must refuse)
    m = h2v.MSMKZG(ctx)
    buf = torch.zeros(32 * n * TR + 64, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    calls = (lambda: b.guards(), lambda: b.guards_into(0, n, mult=buf.data_ptr()), lambda: b.guards_append(None, m))
    for call in calls:                                       # an empty batch (the host form asks for the shape first)
        with pytest.raises(h2v.H2VError, match="nothing uploaded|nothing launched") as e:
            call()
        assert e.value.code == -16
    assert b._lib.h2v_batch_guards(b._h, 0, n, None, None, None, None, None, None) == -16 and "nothing launched" in h2v._lib.last_error()
    b.upload(b"".join(P[:n]), len(P[0]), b"".join(v for inst in I[:n] for col in inst for v in col), [8], None)
    assert b.guard_shape() == (1, TR)                       # valid from the upload on
    for call in calls:                                       # uploaded only: refused, and still uploaded
        with pytest.raises(h2v.H2VError, match="nothing launched"):
            call()
    b.launch()
    lib = b._lib

    def device(first, count, right_scalars=None, status=None):
        return lib.h2v_batch_guards_device(b._h, ctypes.c_size_t(first), ctypes.c_size_t(count), None, None, ctypes.c_void_p(right_scalars), None, None, ctypes.c_void_p(status))

    def refused(match, *a, **k):
        assert device(*a, **k) == -16
        assert "h2v_batch_guards_device" in h2v._lib.last_error() and match in h2v._lib.last_error(), h2v._lib.last_error()
    addr = buf.data_ptr()
    refused("a range outside the upload", 0, n + 1, right_scalars=addr)
    refused("a range outside the upload", n + 1, 0)
    refused("a range outside the upload", 2**63, 2**63, right_scalars=addr)
    refused("d_right_scalars32 is not 16-byte aligned", 0, n, right_scalars=addr + 8)
    refused("d_status is not 16-byte aligned", 0, n, status=addr + 4)
    host = np.zeros(32 * n * TR + 64, dtype=np.uint8)
    refused("d_right_scalars32 is not device memory", 0, n, right_scalars=(host.ctypes.data + 15) // 16 * 16)
    seg = next(x for x in torch.cuda.memory_snapshot() if x["address"] <= addr < x["address"] + x["total_size"])
    end = seg["address"] + seg["total_size"]
    refused("d_right_scalars32: the bytes the call writes end past", 0, n, right_scalars=end - 32 * n * TR + 16)
    assert device(0, 1, status=end - 16) == 0               # what fits: one status word in the allocation's last 16 bytes
    assert device(3, 0, right_scalars=addr + 8) == 0        # count = 0: nothing to do, nothing looked at
    with pytest.raises(ValueError, match="outside the upload"):
        b.guards(4, 5)
    with pytest.raises(ValueError, match="16-byte"):
        b.guards_into(0, n, mult=addr + 8)
    # the launch is unaffected
    ok, st, _, _ = b.finish_groups()
    assert ok == [True] and st == [0] * n
    assert len(b.guards()) == n and len(m) == 0
    m.close(); b.close()


def test_append_refuses_more_than_2_24_terms(pool):
    """An object of 2^24 - 1 terms, made on the device by doubling through add_msm (1 + 2 + .. + 2^23 terms added to it): one more term
    fits exactly, a second does not — by the library's check and by the Python mirror's — and a refusal leaves length and read-back alone"""
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    MAX = h2v.MSMKZG.MAX_TERMS
    assert MAX == 1 << 24
    b = _launched(ctx, P[:4], I[:4], _draws(4, 11), [4])
    rows = b.guards()
    full, power = h2v.MSMKZG(ctx), h2v.MSMKZG(ctx)
    power.append_terms([5], [rows[0]["left_bases"][0]])
    for k in range(24):                                      # power holds 2^k terms
        full.add_msm(power)
        if k < 23:
            with power.clone() as twin:
                power.add_msm(twin)
    power.close()
    assert len(full) == MAX - 1
    tail = lambda: (len(full), full.scalars(len(full) - 3, 3), full.bases(len(full) - 3, 3), full.scalars(0, 2))
    before = tail()
    lib, sz = b._lib, ctypes.c_size_t

    def raw(left, right, first, count):
        return lib.h2v_batch_guards_append(b._h, sz(first), sz(count), left._handle() if left is not None else None,
                                           right._handle() if right is not None else None, None)
    for args in ((full, None, 0, 2), (None, full, 0, 1), (full, None, 1, 3)):
        assert raw(*args) == -16 and "more than 2^24 terms" in h2v._lib.last_error(), args
        assert tail() == before
        with pytest.raises(ValueError, match="2\\^24"):      # the mirror, before the library is asked
            b.guards_append(args[0], args[1], args[2], args[3])
    other = h2v.MSMKZG(ctx)
    assert raw(other, full, 0, 1) == -16 and len(other) == 0 and tail() == before       # both or neither
    assert b.guards_append(full, None, 2, 1) == 0            # exactly 2^24 terms: allowed
    assert len(full) == MAX and full.scalars(MAX - 1, 1) == _ints(rows[2])["left_scalars"] and full.bases(MAX - 1, 1) == rows[2]["left_bases"]
    assert full.scalars(MAX - 4, 3) == before[1] and full.scalars(0, 2) == before[3] == [5, 5]
    assert raw(full, None, 0, 1) == -16 and "more than 2^24 terms" in h2v._lib.last_error() and len(full) == MAX
    assert b.guards_append(full, None, 0, 0) == 0 and len(full) == MAX                   # nothing to add: nothing to refuse
    full.close(); other.close(); b.close()


def test_launch_without_a_pairing(pool):
    """launch(with_pairing=False), what a caller with a strategy of their own does: the accumulators are still in pieces when the
    Guards are asked for; the Guards, and the finish afterwards, are what they are with a pairing"""
    s, P, I, ctx = pool
    n, sizes = 12, [4, 4, 4]
    rand = _draws(n, 12)
    P2 = list(P[:n]); P2[6] = P2[6][:-96] + b"\xff" * 32 + P2[6][-64:]
    b = _launched(ctx, P2, I[:n], rand, sizes, pairing=False)
    got = b.guards()
    _compare(s, got, gr.expected(s, P2, I[:n], rand, sizes))
    paired = _launched(ctx, P2, I[:n], rand, sizes)
    assert paired.guards() == got
    plain = _launched(ctx, P2, I[:n], rand, sizes, pairing=False)
    want = plain.finish_groups()
    assert b.finish_groups() == want and want[1][6] == -5 and b.guards(2, 7) == got[2:9]
    assert (want[2], want[3]) == paired.finish_groups()[2:]
    b.close(); paired.close(); plain.close()


def test_a_smaller_upload_into_a_larger_batch(pool):
    """n < max_proofs, behind a larger upload of other proofs: the addressing follows the upload's n, and nothing of the earlier
    launch shows — its scalars lie where this upload's failing proof and this upload's VK-wide scalars are read"""
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    b = h2v.Batch(ctx, 12, 8)
    b.set_group_sizes([5, 7])
    flat = lambda Ps, Is: (b"".join(Ps), len(Ps[0]), b"".join(v for inst in Is for col in inst for v in col), [8])
    big = _draws(12, 13)
    b.upload(*flat(P[:12], I[:12]), b"".join(r.to_bytes(32, "little") for r in big))
    b.launch()
    _compare(s, b.guards(), gr.expected(s, P[:12], I[:12], big, [5, 7]))
    sizes = [2, 3]
    b.set_group_sizes(sizes)
    P2, I2 = [P[i] for i in (9, 3, 14, 0, 7)], [I[i] for i in (9, 3, 14, 0, 7)]
    P2[1] = P2[1][:-96] + b"\xff" * 32 + P2[1][-64:]         # a failing proof where the first launch left a clean one's scalars
    rand = _draws(5, 14)
    b.upload(*flat(P2, I2), b"".join(r.to_bytes(32, "little") for r in rand))
    b.launch()
    exp = gr.expected(s, P2, I2, rand, sizes)
    got = b.guards()
    _compare(s, got, exp)
    assert got[1]["status"] == -5 and set(got[1]["right_scalars"]) == {bytes(32)}
    _compare(s, b.guards(1, 3), exp[1:4])
    fresh = _launched(ctx, P2, I2, rand, sizes)
    assert fresh.guards() == got and fresh.finish_groups() == b.finish_groups()
    b.close(); fresh.close()


def test_a_device_draw_of_r_is_refused_by_the_forms_that_wait(pool):
    """draws uploaded from device memory with one >= r: the host and the append form refuse in finish's words and hand out nothing, the
    stage stays, and the finish afterwards still reports the draw and leaves the batch empty"""
    import torch
    import halo2_verifier_amd as h2v
    s, P, I, ctx = pool
    n = 8
    rand = _draws(n, 15)
    rand[5] = R_MOD
    proofs = torch.frombuffer(bytearray(b"".join(P[:n])), dtype=torch.uint8).reshape(n, len(P[0])).cuda()
    insts = torch.frombuffer(bytearray(b"".join(v for inst in I[:n] for col in inst for v in col)), dtype=torch.uint8).reshape(n, 256).cuda()
    draws = torch.frombuffer(bytearray(b"".join(r.to_bytes(32, "little") for r in rand)), dtype=torch.uint8).reshape(n, 32).cuda()
    b = h2v.Batch(ctx, n, 8, groups=2)
    b.upload_tensors(proofs, insts, [8], draws)
    b.launch()
    m = h2v.MSMKZG(ctx)
    for call in (lambda: b.guards(), lambda: b.guards(1, 2), lambda: b.guards_append(None, m), lambda: b.guards_append(m, None, 0, 3)):
        with pytest.raises(h2v.H2VError, match="draw 5 ") as e:
            call()
        assert e.value.code == -16 and len(m) == 0
    with pytest.raises(h2v.H2VError, match="draw 5 "):
        b.finish_groups()
    with pytest.raises(h2v.H2VError, match="nothing uploaded|nothing launched"):
        b.guards()
    good = _draws(n, 16)
    draws = torch.frombuffer(bytearray(b"".join(r.to_bytes(32, "little") for r in good)), dtype=torch.uint8).reshape(n, 32).cuda()
    b.upload_tensors(proofs, insts, [8], draws)
    b.launch()
    _compare(s, b.guards(), gr.expected(s, P[:n], I[:n], good, [4, 4]))
    assert b.guards_append(m, None) == 0 and len(m) == n
    m.close(); b.close()
