"""h2v_verify_batches: many AccumulatorStrategy batches of their own sizes in one call.  Batch i's (ok, statuses, left, right) must be
bit for bit what h2v_verify_batch gives over its slice with its draws: for a call of mixed sizes in one launch, for 520 batches (two
launches: a launch holds 512 groups), for a batch above the proof budget of a launch beside small ones, with OS draws, and through the
C++ mirror."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu
LAUNCH_PROOFS = 16384      # H2V_BATCHES_LAUNCH_PROOFS (csrc/oneshot.hip)


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 256, seed=4321, threads=16)
    yield s, P, I
    s.free()


@pytest.fixture(scope="module")
def ctx(pool):
    import halo2_verifier_amd as h2v
    s = pool[0]
    c = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    yield c
    c.close()


def _cut(P, I, sizes):
    """the pool's proofs, cycled, as batches of these sizes"""
    out, at = [], 0
    for sz in sizes:
        idx = [(at + j) % len(P) for j in range(sz)]
        out.append(([P[i] for i in idx], [I[i] for i in idx])); at += sz
    return out


def _rand_per_batch(rand, sizes):
    out, at = [], 0
    for sz in sizes:
        out.append(rand[at:at + sz]); at += sz
    return out


def test_seven_mixed_batches_equal_seven_calls(pool, ctx):
    s, P, I = pool
    sizes = [1, 7, 24, 3, 1, 64, 5]
    batches = _cut(P, I, sizes)
    # batch 2: a wrong public input (only its verdict falls); batch 5: an undecodable point and a short proof (statuses at the right proofs)
    p2, i2 = batches[2]
    i2[11] = [[circuits.le32(5)] + i2[11][0][1:]]
    p5, _ = batches[5]
    bad = bytearray(p5[40]); bad[-33] = 0xff; p5[40] = bytes(bad)
    p5[3] = p5[3][:500]
    rnd = random.Random(61)
    rand = [rnd.randrange(1, R_MOD) for _ in range(sum(sizes))]
    got = ctx.verify_batches(batches, rand)
    assert [r[0] for r in got] == [True, True, False, True, True, False, True]
    assert [i for i, v in enumerate(got[5][1]) if v] == [3, 40]
    for g, ((p, i), r) in enumerate(zip(batches, _rand_per_batch(rand, sizes))):
        assert got[g] == ctx.verify_batch(p, i, r), g
    for g in (0, 2, 5):
        p, i = batches[g]
        if g != 5:     # (the oracle takes whole proofs)
            assert got[g] == circuits.oracle_verify_batch(s, p, i, _rand_per_batch(rand, sizes)[g])


def test_520_batches_make_two_launches(pool, ctx):
    s, P, I = pool
    sizes = [1 + (g % 3 == 1) for g in range(520)]
    batches = _cut(P, I, sizes)
    # two proofs with an undecodable opening point, one in each launch: a status of their own, the same under SingleStrategy
    for g in (100, 515):
        p, _ = batches[g]
        bad = bytearray(p[0]); bad[-33] = 0xff; p[0] = bytes(bad)
    rand = [1] * sum(sizes)
    got = ctx.verify_batches(batches, rand)
    assert [g for g, r in enumerate(got) if not r[0]] == [100, 515]
    flatP, flatI = [x for p, _ in batches for x in p], [x for _, i in batches for x in i]
    statuses = [v for r in got for v in r[1]]
    assert statuses == ctx.verify_each(flatP, flatI) and sum(1 for v in statuses if v) == 2
    for g in (0, 519, 100, 515):
        p, i = batches[g]
        assert got[g] == ctx.verify_batch(p, i, [1] * sizes[g]), g


def test_a_batch_above_the_proof_budget_beside_small_ones(pool, ctx):
    s, P, I = pool
    sizes = [3, LAUNCH_PROOFS + 5, 2, 1]
    batches = _cut(P, I, sizes)
    rnd = random.Random(67)
    rand = [rnd.randrange(1, R_MOD) for _ in range(sum(sizes))]
    got = ctx.verify_batches(batches, rand)
    assert [r[0] for r in got] == [True] * 4
    for g, ((p, i), r) in enumerate(zip(batches, _rand_per_batch(rand, sizes))):
        assert got[g] == ctx.verify_batch(p, i, r), g


def test_os_draws_accept_valid_proofs_and_arguments_are_checked_first(pool, ctx):
    import halo2_verifier_amd as h2v
    s, P, I = pool
    sizes = [2, 9, 1]
    batches = _cut(P, I, sizes)
    got = ctx.verify_batches(batches)
    assert [r[0] for r in got] == [True] * 3 and all(r[1] == [0] * sz for r, sz in zip(got, sizes))
    assert ctx.verify_batches([]) == []
    # the C side's own checks: a zero size, a draw that is no canonical scalar
    m = h2v.verifier._marshal_batch([ctx], [x for p, _ in batches for x in p], [x for _, i in batches for x in i])
    import ctypes
    st, ok = (ctypes.c_int * 12)(), (ctypes.c_int * 3)()
    c_sizes = h2v.verifier._sizes
    assert ctx._lib.h2v_verify_batches(ctx._h, 3, c_sizes([2, 0, 10]), *m.head[1:], m.ncols[0], m.shape0(), None, st, ok, None, None) == -16
    assert ctx._lib.h2v_verify_batches(ctx._h, 3, c_sizes(sizes), *m.head[1:], m.ncols[0], m.shape0(), b"\xff" * (32 * 12), st, ok, None, None) == -16
    assert ctx._lib.h2v_verify_batches(ctx._h, 3, c_sizes(sizes), *m.head[1:], m.ncols[0], m.shape0(), None, st, ok, None, None) == 0 and list(ok) == [1, 1, 1]


def test_cpp_mirror_verify_batches(pool, ctx, tmp_path):
    s, P, I = pool
    exe = ch.build("verify_batches", tmp_path)
    sizes = [4, 1, 9]
    batches = _cut(P, I, sizes)
    p1, i1 = batches[1]
    i1[0] = [[circuits.le32(5)] + i1[0][0][1:]]
    rnd = random.Random(71)
    rand = [rnd.randrange(1, R_MOD) for _ in range(sum(sizes))]
    text = ch.items_text([x for p, _ in batches for x in p], [x for _, i in batches for x in i], header="%d\n%s" % (len(sizes), " ".join(map(str, sizes))))
    d = ch.write_dir(tmp_path, s.params, vk=s.vk, rand=rand, items_txt=text)
    out = ch.run(exe, [d], timeout=120).stdout.splitlines()
    rows = [l.split() for l in out if l.startswith("batch ")]
    assert len(rows) == 3 and "empty_refused -16" in out
    want = ctx.verify_batches(batches, rand)
    assert [r[0] for r in want] == [True, False, True]
    for m, w in zip(rows, want):
        assert ((m[1] == "1"), [int(x) for x in m[4:]], bytes.fromhex(m[2]), bytes.fromhex(m[3])) == w


def test_one_large_batch_beside_511_single_proofs(pool, ctx):
    """A batch whose right-channel MSM problem is above 16 384 terms is cut into two sub-problems, so beside it a launch holds 510 one-proof
    batches, not 511 (1024 sub-problems per launch): the call closes the launch there instead of handing the upload a layout it
    refuses, and every batch still equals verify_batch."""
    s, P, I = pool
    big = 16384 // ctx.proof_shape()["n_points"] + 1
    sizes = [big] + [1] * 511
    batches = _cut(P, I, sizes)
    p, _ = batches[300]
    bad = bytearray(p[0]); bad[-33] = 0xff; p[0] = bytes(bad)
    rnd = random.Random(73)
    rand = [rnd.randrange(1, R_MOD) for _ in range(sum(sizes))]
    got = ctx.verify_batches(batches, rand)
    assert [g for g, r in enumerate(got) if not r[0]] == [300]
    rb = _rand_per_batch(rand, sizes)
    for g in (0, 1, 300, 509, 510, 511):
        p, i = batches[g]
        assert got[g] == ctx.verify_batch(p, i, rb[g]), g
    # the large batch last, and in the middle of more than one launch's worth of small ones
    for sizes in ([1] * 511 + [big], [1] * 600 + [big] + [2] * 30):
        batches = _cut(P, I, sizes)
        rand = [rnd.randrange(1, R_MOD) for _ in range(sum(sizes))]
        got = ctx.verify_batches(batches, rand)
        rb = _rand_per_batch(rand, sizes)
        assert all(r[0] for r in got)
        for g in (0, sizes.index(big) - 1, sizes.index(big), len(sizes) - 1):
            p, i = batches[g]
            assert got[g] == ctx.verify_batch(p, i, rb[g]), g
