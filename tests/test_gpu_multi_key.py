"""One AccumulatorStrategy over proofs of several VerifyingKeys (h2v_verify_batch_keys).

The reference's verify_proof takes params, vk and instances on every call (lib.rs:33-49) and AccumulatorStrategy only ever sees
MSMs (kzg/strategy.rs:125-140), so one accumulation may hold proofs of several circuits over the same SRS and finalize() runs ONE
pairing for all of them.  Expected values come from the oracle's per-proof Guards (circuits.oracle_accumulate): proof i scaled by
the product of the draws of all later proofs in CALL order, whatever their key."""
import ctypes
import random
import threading

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu

BAD_ARGUMENT, UNSUPPORTED, INVALID_INSTANCES = -16, -19, -1


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes),
                       multiopen=s.multiopen, transcript=s.transcript, circuit_instances=s.circuit_instances)


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


def _run(items, setups, ctxs, rand):
    """verify_batch_keys over items = [(setup, proof, instances)], key = the setup's index in `setups`"""
    import halo2_verifier_amd as h2v
    keys = [next(k for k, s in enumerate(setups) if s is it[0]) for it in items]
    return h2v.verify_batch_keys(ctxs, keys, [p for _, p, _ in items], [i for _, _, i in items], rand)


def _interleave(a, b):
    out = []
    for x, y in zip(a, b):
        out += [x, y]
    return out


def _raw(ctxs, keys, proofs, instances, ncols, col_lens, rand=None):
    """h2v_verify_batch_keys with every argument as given (no checks on the Python side) -> (rc, ok, statuses, left, right)"""
    from halo2_verifier_amd import _lib
    lib = _lib.load_library()
    n = len(proofs)
    PA = ctypes.c_char_p * max(n, 1)
    ca = (ctypes.c_void_p * len(ctxs))(*[c._h.value for c in ctxs])
    ka = (ctypes.c_uint32 * max(n, 1))(*keys)
    pl = (ctypes.c_size_t * max(n, 1))(*[len(p) for p in proofs])
    ia = PA(*[b"".join(v for col in inst for v in col) for inst in instances])
    nca = (ctypes.c_size_t * len(ncols))(*ncols)
    cl = (ctypes.c_size_t * max(len(col_lens), 1))(*col_lens)
    rb = b"".join(r.to_bytes(32, "little") for r in rand) if rand is not None else None
    st = (ctypes.c_int * max(n, 1))()
    ok = ctypes.c_int(0)
    left, right = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
    rc = lib.h2v_verify_batch_keys(ca, len(ctxs), ka, n, PA(*proofs), pl, ia, nca, cl, rb, st, ctypes.byref(ok), left, right)
    return rc, bool(ok.value), list(st)[:n], left.raw, right.raw


def _mixed_lens(s, lens, seed):
    rnd = random.Random(seed)
    P, I = [], []
    for j, m in enumerate(lens):
        a = [rnd.randrange(R_MOD) for _ in range(s.n_mul)]
        b = [rnd.randrange(R_MOD) for _ in range(m)] + [0] * (s.n_mul - m)
        p, inst = circuits.prove_vector_mul_len(s, a, b, m, rng_seed=seed * 100 + j)
        P.append(p); I.append(inst)
    return P, I


@pytest.fixture(scope="module")
def two_keys():
    """vector-mul with n_mul 8 and 4 over one params, 32 proofs each, and a context per key"""
    s8, s4 = circuits.setup_vector_mul(8, 8), circuits.setup_vector_mul(8, 4)
    assert s8.params == s4.params and s8.vk != s4.vk
    P8, I8 = circuits.prove_vector_mul_batch(s8, 32, seed=31, threads=8)
    P4, I4 = circuits.prove_vector_mul_batch(s4, 32, seed=32, threads=8)
    c8, c4 = _ctx(s8), _ctx(s4)
    yield s8, s4, list(zip(P8, I8)), list(zip(P4, I4)), c8, c4
    c8.close(); c4.close()
    s8.free(); s4.free()


def test_two_vector_mul_keys_interleaved(two_keys):
    s8, s4, A, B, c8, c4 = two_keys
    items = _interleave([(s8, p, i) for p, i in A], [(s4, p, i) for p, i in B])
    assert len(items) == 64
    rand = _draws(64, 1)
    exp = circuits.oracle_accumulate(items, rand)
    assert exp[0] is True
    assert _run(items, [s8, s4], [c8, c4], rand) == exp
    # the keys listed the other way round: the same accumulation
    assert _run(items, [s4, s8], [c4, c8], rand) == exp
    # runs of one key, then the other, then the first again
    items = items[:10] + sorted(items[10:40], key=lambda it: it[0] is s4) + items[40:]
    exp = circuits.oracle_accumulate(items, rand)
    assert _run(items, [s8, s4], [c8, c4], rand) == exp


def test_three_circuit_families_with_their_own_options():
    sv = circuits.setup_vector_mul(8, 6)
    ssh = circuits.setup_shuffle(8, s_seed=42).set_options(circuits.GWC, circuits.KECCAK256)
    sw = circuits.setup_wide(8, s_seed=42).set_circuit_instances(2)
    assert sv.params == ssh.params == sw.params
    Pv, Iv = circuits.prove_vector_mul_batch(sv, 6, seed=41, threads=4)
    items_v = [(sv, p, i) for p, i in zip(Pv, Iv)]
    items_sh = [(ssh, *circuits.prove_shuffle(ssh, data_seed=5 + j, rng_seed=90 + j)) for j in range(4)]
    items_w = [(sw, *circuits.prove_wide_multi(sw, 2, witness_seed=3 + j, rng_seed=130 + j)) for j in range(3)]
    items = [items_v[0], items_sh[0], items_w[0], items_v[1], items_v[2], items_sh[1], items_w[1], items_sh[2], items_v[3],
             items_w[2], items_v[4], items_sh[3], items_v[5]]
    rand = _draws(len(items), 2)
    exp = circuits.oracle_accumulate(items, rand)
    assert exp[0] is True
    ctxs = [_ctx(sv), _ctx(ssh), _ctx(sw)]
    assert _run(items, [sv, ssh, sw], ctxs, rand) == exp
    for c in ctxs:
        c.close()
    for s in (sv, ssh, sw):
        s.free()


def test_per_proof_shapes_inside_a_key(two_keys):
    s8, s4, A, B, c8, c4 = two_keys
    P, I = _mixed_lens(s8, [8, 5, 8, 3, 5, 0, 8, 3], 9)
    items = []
    for j, (p, i) in enumerate(zip(P, I)):
        items += [(s8, p, i), (s4, *B[j])]
    rand = _draws(len(items), 3)
    exp = circuits.oracle_accumulate(items, rand)
    assert exp[0] is True
    assert _run(items, [s8, s4], [c8, c4], rand) == exp      # 5 groups: 4 shapes of the first key, 1 of the second


def test_failures_on_either_key(two_keys):
    s8, s4, A, B, c8, c4 = two_keys
    items = _interleave([(s8, p, i) for p, i in A[:12]], [(s4, p, i) for p, i in B[:12]])
    rand = _draws(len(items), 4)
    # a tampered public input on the second key: rejected by the pairing only
    bad = list(items)
    s, p, i = bad[5]
    assert s is s4
    bad[5] = (s, p, [[circuits.le32(3)] + i[0][1:]])
    exp = circuits.oracle_accumulate(bad, rand)
    assert exp[0] is False and exp[1] == [0] * len(bad)
    assert _run(bad, [s8, s4], [c8, c4], rand) == exp
    # a truncated proof and a non-canonical scalar on the first key: the last evaluation, read before SHPLONK's h1 and h2 (the proof's
    # last 64 bytes).  Each gets the oracle's status and contributes nothing (oracle_accumulate leaves out the Guard of a failed proof)
    bad = list(items)
    s, p, i = bad[2]
    assert s is s8
    bad[2] = (s, p[:len(p) // 2], i)
    s, p, i = bad[8]
    bad[8] = (s, p[:-96] + b"\xff" * 32 + p[-64:], i)
    exp = circuits.oracle_accumulate(bad, rand)
    assert exp[1][2] != 0 and exp[1][8] != 0 and exp[0] is False
    assert _run(bad, [s8, s4], [c8, c4], rand) == exp


def test_one_key_equals_the_single_key_calls(two_keys):
    import halo2_verifier_amd as h2v
    s8, s4, A, B, c8, c4 = two_keys
    P, I = [p for p, _ in A[:20]], [i for _, i in A[:20]]
    rand = _draws(20, 5)
    want = c8.verify_batch(P, I, rand)                                    # h2v_verify_batch
    assert want[0] is True
    assert h2v.verify_batch_keys([c8], [0] * 20, P, I, rand) == want
    assert h2v.verify_batch_keys([c8, c4], [0] * 20, P, I, rand) == want  # a key no proof uses
    Pm, Im = _mixed_lens(s8, [8, 3, 8, 5, 3], 6)
    rand = _draws(5, 6)
    want = c8.verify_batch(Pm, Im, rand)                                  # h2v_verify_batch_shapes
    assert want[0] is True
    assert h2v.verify_batch_keys([c8], [0] * 5, Pm, Im, rand) == want
    assert h2v.verify_batch_keys([c4, c8], [1] * 5, Pm, Im, rand) == want
    # no proof at all: what h2v_verify_batch gives for n == 0
    assert h2v.verify_batch_keys([c8, c4], [], [], []) == c8.verify_batch([], [])


def test_keys_at_different_k():
    s8 = circuits.setup_vector_mul(8, 6, s_seed=42)
    s9 = circuits.setup_vector_mul(9, 4, s_seed=42)
    # RawBytes params: k, g[0..n), g_lagrange[0..n), g2, s_g2 — the accumulation reads g[0], g2 and s_g2 only
    assert s8.params[4:68] == s9.params[4:68] and s8.params[-256:] == s9.params[-256:] and s8.params != s9.params
    P8, I8 = circuits.prove_vector_mul_batch(s8, 6, seed=61, threads=4)
    P9, I9 = circuits.prove_vector_mul_batch(s9, 6, seed=62, threads=4)
    items = _interleave([(s8, p, i) for p, i in zip(P8, I8)], [(s9, p, i) for p, i in zip(P9, I9)])
    rand = _draws(len(items), 7)
    exp = circuits.oracle_accumulate(items, rand)
    assert exp[0] is True
    ctxs = [_ctx(s8), _ctx(s9)]
    assert _run(items, [s8, s9], ctxs, rand) == exp
    for c in ctxs:
        c.close()
    s8.free(); s9.free()


def test_refusals_leave_every_context_usable(two_keys):
    s8, s4, A, B, c8, c4 = two_keys
    P, I = [p for p, _ in A[:4]] + [p for p, _ in B[:4]], [i for _, i in A[:4]] + [i for _, i in B[:4]]
    keys = [0] * 4 + [1] * 4
    col_lens = [8] * 4 + [4] * 4

    def still_good():
        for s, c, items in ((s8, c8, A[:6]), (s4, c4, B[:6])):
            rand = _draws(6, 8)
            exp = circuits.oracle_verify_batch(s, [p for p, _ in items], [i for _, i in items], rand)
            assert exp[0] is True and c.verify_batch([p for p, _ in items], [i for _, i in items], rand) == exp

    assert _raw([c8, c4], keys, P, I, [1, 1], col_lens, _draws(8, 9))[0] == 0
    other = circuits.setup_vector_mul(8, 4, s_seed=43)                   # params over another s
    co = _ctx(other)
    assert _raw([c8, co], keys, P, I, [1, 1], col_lens)[0] == BAD_ARGUMENT
    still_good()
    assert _raw([c8, c8], keys, P, I, [1, 1], col_lens)[0] == BAD_ARGUMENT                       # a repeated context
    still_good()
    assert _raw([c8, c4], keys[:-1] + [2], P, I, [1, 1], col_lens)[0] == BAD_ARGUMENT             # a key index out of range
    still_good()
    assert _raw([c8, c4], keys, P, I, [1, 2], col_lens + [4] * 4)[0] == INVALID_INSTANCES          # a wrong n_instance_columns
    still_good()
    # 65 (key, shape) groups: refused before anything runs, so the proofs need not verify
    keys65 = [0] * 64 + [1]
    lens65 = list(range(64)) + [4]
    I65 = [[[circuits.le32(1)] * m] for m in lens65]
    assert _raw([c8, c4], keys65, [P[0]] * 65, I65, [1, 1], lens65)[0] == UNSUPPORTED
    still_good()
    co.close(); other.free()


def test_a_thousand_proofs_over_two_keys(two_keys):
    import halo2_verifier_amd as h2v
    s8, s4, A, B, c8, c4 = two_keys
    n = 1100
    items = [(s8, *A[(k // 2) % len(A)]) if k % 2 == 0 else (s4, *B[(k // 3) % len(B)]) for k in range(n)]
    keys = [0 if s is s8 else 1 for s, _, _ in items]
    P, I = [p for _, p, _ in items], [i for _, _, i in items]
    ok, st, _, _ = h2v.verify_batch_keys([c8, c4], keys, P, I)          # OS draws: the verdict only
    assert ok is True and st == [0] * n
    rand = _draws(n, 10)
    exp = circuits.oracle_accumulate(items, rand)
    assert exp[0] is True
    assert h2v.verify_batch_keys([c8, c4], keys, P, I, rand) == exp


def test_two_threads_with_the_keys_in_opposite_orders(two_keys):
    import halo2_verifier_amd as h2v
    s8, s4, A, B, c8, c4 = two_keys
    items = _interleave([(s8, p, i) for p, i in A[:16]], [(s4, p, i) for p, i in B[:16]])
    P, I = [p for _, p, _ in items], [i for _, _, i in items]
    rand = _draws(len(items), 11)
    exp = circuits.oracle_accumulate(items, rand)
    keys = [0 if s is s8 else 1 for s, _, _ in items]
    results = {"ab": [], "ba": []}

    def worker(name, ctxs, kk):
        for _ in range(4):
            results[name].append(h2v.verify_batch_keys(ctxs, kk, P, I, rand))

    ta = threading.Thread(target=worker, args=("ab", [c8, c4], keys))
    tb = threading.Thread(target=worker, args=("ba", [c4, c8], [1 - k for k in keys]))
    ta.start(); tb.start()
    ta.join(timeout=240); tb.join(timeout=240)
    assert not ta.is_alive() and not tb.is_alive(), "deadlock"
    assert results["ab"] == [exp] * 4 and results["ba"] == [exp] * 4


def test_python_accumulator_strategy_over_two_vks(two_keys):
    import halo2_verifier_amd as h2v
    s8, s4, A, B, c8, c4 = two_keys
    items = _interleave([(s8, p, i) for p, i in A[:9]], [(s4, p, i) for p, i in B[:9]])
    rand = _draws(len(items), 12)
    params = h2v.ParamsKZG(s8.params, h2v.SerdeFormat.RawBytes)
    vks = {id(s8): h2v.VerifyingKey(s8.vk, h2v.SerdeFormat.RawBytes), id(s4): h2v.VerifyingKey(s4.vk, h2v.SerdeFormat.RawBytes)}
    strat = h2v.AccumulatorStrategy(params, rand=rand)
    for s, p, i in items:
        strat = h2v.verify_proof(params, vks[id(s)], strat, i, p)
    exp = circuits.oracle_accumulate(items, rand)
    assert exp[0] is True
    assert strat.finalize() is True
    assert (strat.left_xy, strat.right_xy) == (exp[2], exp[3])
    # a seeded accumulation over two VKs stays refused
    seeded = h2v.AccumulatorStrategy.with_accumulator(params, ([1], [exp[2]]), ([1], [exp[3]]), rand=rand)
    for s, p, i in items:
        seeded = h2v.verify_proof(params, vks[id(s)], seeded, i, p)
    with pytest.raises(ValueError):
        seeded.finalize()
