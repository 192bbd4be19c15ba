"""The C++ mirror of the merge of resident accumulators (include/h2v.hpp Accumulator::merge / export_state / merge_states) through the
C ABI: tests/cpp/merge_harness.cpp feeds ten proofs to three accumulators, merges them into a journaled one — directly, through
their exported states, and with draws of the library's own — and prints the bytes; every line is compared with the Python class on
the same proofs and with the CPU oracle's merge."""
import random

import pytest

import caller_harness as ch
import circuits
import merge_reference as mr
import oracle_lib
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_merge_of_three_accumulators(tmp_path):
    import halo2_verifier_amd as h2v
    exe = ch.build("merge_harness", tmp_path)
    n, K = 10, 3
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, n, seed=61, threads=4)
    P[4] = P[4][:-96] + b"\xff" * 32 + P[4][-64:]                    # a non-canonical scalar: status -5, on source 1
    rnd = random.Random(62)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    draws = [rnd.randrange(1, R_MOD) for _ in range(K)]
    d = ch.write_dir(tmp_path, s.params, vks=[s.vk], rand=rand, draws_bin=ch.draws(draws), items_txt=ch.items_text(P, I, keys=[0] * n))
    out = ch.run(exe, [d, K]).stdout.splitlines()

    # the oracle: every source alone, then the merge
    L = oracle_lib.load()
    owns = [circuits.oracle_accumulate([(s, P[i], I[i]) for i in range(k, n, K)], rand[k::K]) for k in range(K)]
    exp_states = [mr.pack_state(o[2], o[3], len(o[1]), sum(1 for v in o[1] if v)) for o in owns]
    assert [sum(1 for v in o[1] if v) for o in owns] == [0, 1, 0]

    def merged(cs):
        return oracle_lib.g1_msm(L, cs, [o[2] for o in owns]), oracle_lib.g1_msm(L, cs, [o[3] for o in owns])

    left, right = merged(draws)
    assert circuits.oracle_pairing_check(s, left, right) is True
    want = ["0", left.hex(), right.hex(), str(n), "1", str(K + 1), b"".join(c.to_bytes(32, "little") for c in draws).hex()]   # not ok: the failed status

    # the Python class on the same proofs
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    srcs = []
    for k in range(K):
        a = h2v.Accumulator(ctx)
        a.process(ctx, None, P[k::K], I[k::K], rand[k::K])
        srcs.append(a)
    py_states = [a.export_state() for a in srcs]
    dst = h2v.Accumulator(ctx, journal=K + 1)
    used = dst.merge(srcs, draws)
    py = [str(int(dst.finalize()[0])), dst.read()[0].hex(), dst.read()[1].hex(), str(dst.read()[2]), str(dst.read()[3]), str(len(dst.check_legs())), b"".join(used).hex()]
    for a in srcs + [dst]:
        a.close()
    ctx.close()

    assert [bytes.fromhex(l.split()[2]) for l in out if l.startswith("state ")] == py_states == exp_states
    assert [l for l in out if l.startswith("merge ")][0].split()[1:] == py == want
    assert [l for l in out if l.startswith("states ")][0].split()[1:] == want
    drawn = [l for l in out if l.startswith("drawn ")][0].split()
    cs = [int.from_bytes(bytes.fromhex(drawn[3])[32 * k:32 * k + 32], "little") for k in range(K)]
    assert drawn[1:3] == ["0", str(n)] and all(0 < c < R_MOD for c in cs) and len(set(cs)) == K
    assert [l for l in out if l.startswith(("refused", "accepted"))] == [
        "refused too many sources", "refused draws of a wrong length", "refused states of a wrong length", "refused too many states",
        "refused the destination as a source", "refused a null source"]
    s.free()
