"""Hint rows from SOME senders, through the C ABI and its Python mirror (include/h2v_hint_rows.h; halo2_verifier_amd/hints.py):
h2v_batch_set_hint_rows, h2v_verify_batch_keys_hinted, h2v_verify_batches_hinted, h2v_accumulator_process_hinted, and the sharded
calls' hints= keyword.

The invariant under test is include/h2v_hints.h's: the results depend on the proofs, instances and draws only.  Every case compares a
call with hint rows byte for byte with the same call without them over the same proofs and draws — statuses, verdicts, both
accumulator points, the resident accumulator's points and counters — and the three counters (points, hinted points, hinted points
missed) with the counts tests/hints_reference.py gives.  A proof without a row counts neither as hinted nor as missed, and neither does
a proof shorter than its key's proof, whatever row came with it.

Proofs: 70 of the k = 8 vector-mul circuit of tests/circuits.py (840 points, 14 waves of the decompression), and 6 of the shuffle
circuit over the same params, whose key has another number of points.  Row variants: (a) every row right, (b) every second row None,
(c) random bytes, (d) right rows around one tampered proof (only the pairing rejects it), one short proof and one undecodable point."""
import ctypes
import random

import pytest

import circuits
import hints_reference as hr
from circuits import R_MOD

pytestmark = pytest.mark.gpu

N = 70
BAD = -16
VARIANTS = ("right", "half", "random", "bad_proofs")


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript, circuit_instances=s.circuit_instances)


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


def _rows(off, proofs):
    """the right row of every proof -> list of bytes"""
    return [hr.rows(off, [p]) for p in proofs]


def _variant(kind, off, P, short=True):
    """-> (proofs, rows) of a row variant over the proofs P of a key whose points lie at `off`.  short: (d) may hold a short proof (a
    staged batch takes none)"""
    P = list(P)
    rows = _rows(off, P)
    if kind == "half":
        rows = [r if i % 2 == 0 else None for i, r in enumerate(rows)]
    elif kind == "random":
        rnd = random.Random(len(P))
        rows = [bytes(rnd.randrange(256) for _ in range(len(r))) for r in rows]
    elif kind == "bad_proofs" and len(P) >= 3:
        n = len(P)
        scalar_at = max(o for o in range(0, len(P[0]) - 32, 32) if o not in off)       # an evaluation: only the pairing rejects the proof
        a, b, c = n // 3, n // 2, n - 2
        bad = bytearray(P[a]); bad[scalar_at] ^= 1; P[a] = bytes(bad)
        bad = bytearray(P[c]); bad[off[-1]:off[-1] + 32] = hr.encode(hr.non_residue_x(4242), 1); P[c] = bytes(bad)
        rows = _rows(off, P)                                                               # (the undecodable point's hint: zeros, a miss)
        if short:
            P[b] = P[b][:off[len(off) // 2] + 7]                                           # the reader runs dry inside a point; its row stays the whole proof's
    return P, rows


def _want_stats(items):
    """items: (point offsets of the proof's key, proof, row or None) -> the three counters.  A short proof is a proof without a row."""
    points = hinted = missed = 0
    for off, proof, row in items:
        points += len(off)
        if row is None or len(proof) < off[-1] + 32:
            continue
        hinted += len(off)
        missed += hr.count_misses(hr.points_of(off, proof), row)
    return points, hinted, missed


@pytest.fixture(scope="module")
def pool():
    from halo2_verifier_amd import hints
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, N, seed=1848, threads=16)
    c = _ctx(s)
    off = hints.point_offsets(c)
    yield dict(s=s, P=P, I=I, ctx=c, off=off, np=len(off), rand=_draws(N, 7))
    c.close()
    s.free()


@pytest.fixture(scope="module")
def other_key(pool):
    """six proofs of the shuffle circuit over the same params: a key with another number of points"""
    from halo2_verifier_amd import hints
    s = circuits.setup_shuffle(8, s_seed=42)
    assert s.params == pool["s"].params
    proofs = [circuits.prove_shuffle(s, data_seed=5 + i, rng_seed=9 + i) for i in range(6)]
    c = _ctx(s)
    off = hints.point_offsets(c)
    assert len(off) != pool["np"]
    yield dict(s=s, P=[p for p, _ in proofs], I=[i for _, i in proofs], ctx=c, off=off)
    c.close()
    s.free()


# ------------------------------------------------------------------ the staged batch
def _staged(ctx, P, I, rand, rows=None, keep=False):
    import halo2_verifier_amd as h2v
    b = h2v.Batch(ctx, len(P), 64)
    b.upload(b"".join(P), len(P[0]), b"".join(b"".join(col) for i in I for col in i), [len(col) for col in I[0]], b"".join(r.to_bytes(32, "little") for r in rand))
    if rows is not None:
        b.set_hint_rows(rows)
    b.launch()
    out = b.finish_groups(), b.hint_stats()
    if keep:
        return out + (b,)
    b.close()
    return out


@pytest.mark.parametrize("kind", VARIANTS)
def test_a_staged_batch_with_hint_rows(pool, kind):
    c, I, rand, off = pool["ctx"], pool["I"], pool["rand"], pool["off"]
    P, rows = _variant(kind, off, pool["P"], short=False)
    plain, plain_stats = _staged(c, P, I, rand)
    got, stats, b = _staged(c, P, I, rand, rows, keep=True)
    assert got == plain and plain_stats == (N * len(off), 0, 0)
    want = _want_stats([(off, p, r) for p, r in zip(P, rows)])
    print(kind, "hint stats", stats, "reference", want)
    assert stats == want
    if kind == "half":
        assert stats[1] == 35 * len(off) and stats[2] == 0          # n_hinted = 35 x Np; the 35 proofs without a row are not misses
    if kind == "bad_proofs":
        assert got[0] == [False] and got[1][N - 2] == -4 and stats[2] == 1
    assert b.hints() == hr.rows(off, P)                             # what the launch leaves: the canonical rows of ALL proofs
    b.close()


def test_set_hint_rows_keeps_set_hints_rules(pool):
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import hints
    c, P, I, rand, off = pool["ctx"], pool["P"][:9], pool["I"][:9], pool["rand"][:9], pool["off"]
    lib = hints._library()
    rows = _rows(off, P)
    arr = (ctypes.c_char_p * 9)(*rows)
    b = h2v.Batch(c, 9, 64)
    assert lib.h2v_batch_set_hint_rows(b._h, 9, arr) == BAD and "h2v_batch_set_hint_rows" in h2v._lib.last_error()      # before any upload
    upload = lambda: b.upload(b"".join(P), len(P[0]), b"".join(b"".join(col) for i in I for col in i), [8], b"".join(r.to_bytes(32, "little") for r in rand))
    upload()
    assert lib.h2v_batch_set_hint_rows(b._h, 8, arr) == BAD and lib.h2v_batch_set_hint_rows(b._h, 10, arr) == BAD        # n != the upload's
    b.set_hint_rows(rows)
    b.set_hint_rows(None)                                                    # dropped: an unhinted launch
    b.launch()
    plain = b.finish_groups()
    assert b.hint_stats() == (9 * len(off), 0, 0)
    assert lib.h2v_batch_set_hint_rows(b._h, 9, arr) == BAD                  # after a launch
    upload()
    b.set_hint_rows([None] * 9)                                              # nobody gave a row: no hints
    b.launch()
    assert (b.finish_groups(), b.hint_stats()) == (plain, (9 * len(off), 0, 0))
    upload()
    b.set_hint_rows([rows[0]] + [None] * 8)
    b.launch()
    assert (b.finish_groups(), b.hint_stats()) == (plain, (9 * len(off), len(off), 0))
    b.launch()                                                               # a relaunch finds the canonical y of ALL points where the rows lay: every point hinted
    assert (b.finish_groups(), b.hint_stats()) == (plain, (9 * len(off), 9 * len(off), 0))
    upload()
    b.set_hints(b"".join(rows))                                              # and set_hints reports what it reported
    b.launch()
    assert (b.finish_groups(), b.hint_stats()) == (plain, (9 * len(off), 9 * len(off), 0))
    b.close()


# ------------------------------------------------------------------ h2v_verify_batch_keys_hinted
@pytest.mark.parametrize("kind", VARIANTS)
def test_verify_batch_with_hint_rows(pool, kind):
    c, I, rand, off = pool["ctx"], pool["I"], pool["rand"], pool["off"]
    P, rows = _variant(kind, off, pool["P"])
    plain = c.verify_batch(P, I, rand)
    assert c.verify_batch(P, I, rand, hints=rows) == plain
    want = _want_stats([(off, p, r) for p, r in zip(P, rows)])
    print(kind, "hint stats", c.last_hint_stats, "reference", want)
    assert c.last_hint_stats == want
    if kind == "right":
        assert plain[0] and want == (N * len(off), N * len(off), 0)
        ok, st, left, right = circuits.oracle_verify_batch(pool["s"], P, I, rand)
        assert plain == (ok, st, left, right)
    if kind == "half":
        assert want == (N * len(off), 35 * len(off), 0)
    if kind == "bad_proofs":
        assert not plain[0] and plain[1][N // 2] in (-5, -4) and plain[1][N - 2] == -4 and want[1] == (N - 1) * len(off) and want[2] == 1


def test_a_null_row_array_is_the_unhinted_call(pool):
    import halo2_verifier_amd as h2v
    c, P, I, rand = pool["ctx"], pool["P"][:5], pool["I"][:5], pool["rand"][:5]
    plain = c.verify_batch(P, I, rand)
    assert c.verify_batch(P, I, rand, hints=[None] * 5) == plain and c.last_hint_stats == (5 * pool["np"], 0, 0)
    assert h2v.verify_batch_keys([c], [0] * 5, P, I, rand, hints=[None] * 5) == plain + ((5 * pool["np"], 0, 0),)
    assert c.verify_batch([], [], None, hints=[]) == c.verify_batch([], [], None) and c.last_hint_stats == (0, 0, 0)
    # the C entry point with hint_rows NULL: the call IS the unhinted one, and counts its points
    from halo2_verifier_amd import hints, verifier
    args, _, _ = verifier._keyed_args([c], [0] * 5, P, I, rand)
    r, stats = verifier._Results(5), hints.stats_out()
    assert hints._library().h2v_verify_batch_keys_hinted(*args[:6], None, *args[6:], r.st, ctypes.byref(r.ok), r.left, r.right, stats) == 0
    assert r.result() == plain and tuple(stats) == (5 * pool["np"], 0, 0)
    assert hints._library().h2v_verify_batch_keys_hinted(*args[:6], None, *args[6:], r.st, ctypes.byref(r.ok), r.left, r.right, None) == 0 and r.result() == plain


def test_two_keys_in_one_call_and_in_one_process(pool, other_key):
    """rows of 32 x Np bytes with Np of each proof's own key, interleaved; a row for every second proof"""
    import halo2_verifier_amd as h2v
    A, B = pool, other_key
    items = []
    for i in range(6):
        items += [(0, A["P"][i], A["I"][i], A["off"]), (1, B["P"][i], B["I"][i], B["off"])]
    items += [(0, A["P"][i], A["I"][i], A["off"]) for i in range(6, 40)]
    keys, P, I = [k for k, _, _, _ in items], [p for _, p, _, _ in items], [i for _, _, i, _ in items]
    rows = [hr.rows(off, [p]) if j % 3 else None for j, (_, p, _, off) in enumerate(items)]
    rand = _draws(len(items), 11)
    ctxs = [A["ctx"], B["ctx"]]
    want = _want_stats([(off, p, r) for (_, p, _, off), r in zip(items, rows)])
    assert 0 < want[1] < want[0] and want[2] == 0
    plain = h2v.verify_batch_keys(ctxs, keys, P, I, rand)
    assert plain[0] and h2v.verify_batch_keys(ctxs, keys, P, I, rand, hints=rows) == plain + (want,)
    # the resident accumulator over the same proofs, in two calls
    accs = []
    for hinted in (False, True):
        acc = h2v.Accumulator(ctxs[0])
        st, stats = [], [0, 0, 0]
        for lo, hi in ((0, 17), (17, len(items))):
            st += acc.process(ctxs, keys[lo:hi], P[lo:hi], I[lo:hi], rand[lo:hi], hints=rows[lo:hi] if hinted else None)
            if hinted:
                stats = [x + y for x, y in zip(stats, acc.last_hint_stats)]
        accs.append((st, acc.read(), acc.finalize(), acc.last_all_ok))
        acc.close()
        if hinted:
            assert tuple(stats) == want
    assert accs[0] == accs[1] and accs[0][2][0]
    # a row of the other key's length is refused before anything runs
    wrong = list(rows); wrong[1], wrong[2] = rows[2], rows[1]
    with pytest.raises(ValueError, match="hint row"):
        h2v.verify_batch_keys(ctxs, keys, P, I, rand, hints=wrong)


def test_several_instance_shapes_of_one_key(pool):
    """the hinted h2v_verify_batch_shapes: one context, key_of_proof all zero, two instance shapes"""
    s, c, off = pool["s"], pool["ctx"], pool["off"]
    rnd = random.Random(3)
    P, I = [], []
    for j, m in enumerate((8, 5, 8, 5, 3, 8)):
        a = [rnd.randrange(R_MOD) for _ in range(s.n_mul)]
        b = [rnd.randrange(R_MOD) for _ in range(m)] + [0] * (s.n_mul - m)
        p, inst = circuits.prove_vector_mul_len(s, a, b, m, rng_seed=300 + j)
        P.append(p); I.append(inst)
    rand = _draws(6, 5)
    rows = [r if j != 2 else None for j, r in enumerate(_rows(off, P))]
    plain = c.verify_batch(P, I, rand)
    assert plain[0] and c.verify_batch(P, I, rand, hints=rows) == plain and c.last_hint_stats == (6 * len(off), 5 * len(off), 0)


def test_the_accumulator_strategy_hands_its_rows_on(pool):
    import halo2_verifier_amd as h2v
    s, P, I, rand, off = pool["s"], pool["P"][:7], pool["I"][:7], pool["rand"][:7], pool["off"]
    params, vk = h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes)
    out = []
    for hinted in (False, True):
        strategy = h2v.AccumulatorStrategy(params, rand=rand)
        for j, (p, i) in enumerate(zip(P, I)):
            strategy = h2v.verify_proof(params, vk, strategy, i, p, hints=hr.rows(off, [p]) if hinted and j % 2 else None)
        out.append((strategy.finalize(), strategy.left_xy, strategy.right_xy))
    assert out[0] == out[1] and out[0][0]


# ------------------------------------------------------------------ h2v_verify_batches_hinted
@pytest.mark.parametrize("kind", VARIANTS)
def test_verify_batches_with_hint_rows(pool, kind):
    """three batches of 1, 5 and 64 proofs in one call"""
    c, I, rand, off = pool["ctx"], pool["I"], pool["rand"], pool["off"]
    P, rows = _variant(kind, off, pool["P"])
    cut = [(0, 1), (1, 6), (6, 70)]
    batches = [(P[lo:hi], I[lo:hi]) for lo, hi in cut]
    plain = c.verify_batches(batches, rand)
    assert c.verify_batches(batches, rand, hints=rows) == plain
    assert c.last_hint_stats == _want_stats([(off, p, r) for p, r in zip(P, rows)])
    assert [r[0] for r in plain] == ([True, True, True] if kind != "bad_proofs" else [True, True, False])
    for (lo, hi), res in zip(cut[:2], plain):                         # and a batch of the call is its own verify_batch
        assert res == c.verify_batch(P[lo:hi], I[lo:hi], rand[lo:hi])


# ------------------------------------------------------------------ h2v_accumulator_process_hinted
@pytest.mark.parametrize("kind", VARIANTS)
def test_accumulator_process_with_hint_rows(pool, kind):
    import halo2_verifier_amd as h2v
    c, I, rand, off = pool["ctx"], pool["I"], pool["rand"], pool["off"]
    P, rows = _variant(kind, off, pool["P"])
    seen = []
    for hints in (None, rows):
        acc = h2v.Accumulator(c)
        st = acc.process(c, None, P, I, rand, hints=hints)
        seen.append((st, acc.last_all_ok, acc.read(), acc.finalize()))
        if hints is not None:
            assert acc.last_hint_stats == _want_stats([(off, p, r) for p, r in zip(P, rows)])
        acc.close()
    assert seen[0] == seen[1]
    assert seen[0][1] == (kind != "bad_proofs")


# ------------------------------------------------------------------ sharded
def test_sharded_local_with_hint_rows(pool):
    from halo2_verifier_amd import distributed
    c, P, I, rand, off = pool["ctx"], pool["P"], pool["I"], pool["rand"], pool["off"]
    _, rows = _variant("half", off, P)
    plain = c.verify_batch(P, I, rand)
    assert distributed.verify_batch_sharded_local(c, P, I, rand, world=3, hints=rows) == plain
    assert distributed.verify_batch_sharded_local(c, P, I, rand, world=3) == plain
    assert distributed.verify_batch_sharded(c, P, I, rand, hints=rows) == plain          # a world of one
    with pytest.raises(ValueError, match="70 hint rows"):
        distributed.verify_batch_sharded_local(c, P, I, rand, world=3, hints=rows[:-1])
