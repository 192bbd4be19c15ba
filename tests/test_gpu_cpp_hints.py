"""The C++ mirror (include/h2v_hints.hpp) of point hints, end to end on 5 proofs: tests/cpp/hints_harness.cpp launches one batch without
hints, with the hints h2v::hints::for_proofs makes, with the rows the first launch left (from device memory, padded rows) and with
all-zero hints; the four results must agree with each other and with Batch in Python, the rows with tests/hints_reference.py."""
import random

import pytest

import caller_harness as ch
import circuits
import hints_reference as hr
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_hints_end_to_end(tmp_path):
    import halo2_verifier_amd as h2v
    exe = ch.build("hints_harness", tmp_path, hip=True)
    s = circuits.setup_vector_mul(8, 8)
    n = 5
    P, I = circuits.prove_vector_mul_batch(s, n, seed=277, threads=4)
    rnd = random.Random(278)
    rand = b"".join(rnd.randrange(1, R_MOD).to_bytes(32, "little") for _ in range(n))
    flat, inst = b"".join(P), b"".join(b"".join(col) for i in I for col in i)
    d = ch.write_dir(tmp_path, s.params, vk=s.vk, rand=rand, proofs_bin=flat, instances_bin=inst)
    out = ch.run(exe, [d, n, 1, len(P[0]), 8]).stdout.splitlines()
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    off = h2v.hints.point_offsets(ctx)
    assert out[0] == "offsets " + " ".join(str(o) for o in off), out[0]
    lines = {l.split()[0]: l.split(" ", 1)[1] for l in out[1:] if l.split()[0] in ("plain", "host", "device", "zero")}
    results = {k: v.split(" | ")[0] for k, v in lines.items()}
    stats = {k: tuple(int(x) for x in v.split(" | ")[1].split()) for k, v in lines.items()}
    assert results["plain"] == results["host"] == results["device"] == results["zero"]
    total = n * len(off)
    assert stats == {"plain": (total, 0, 0), "host": (total, total, 0), "device": (total, total, 0), "zero": (total, total, total)}
    assert ch.lines(out, "refused") == ["refused -16"] * 2 and ch.lines(out, "rows") == ["rows same same"]
    b = h2v.Batch(ctx, n, 8)
    b.upload(flat, len(P[0]), inst, [8], rand)
    b.set_hints(h2v.hints.for_proofs(off, flat, len(P[0])))
    b.launch()
    ok, st, left, right = b.finish_groups()
    assert results["plain"].split() == ["".join(str(int(v)) for v in ok)] + [str(v) for v in st] + [left[0].hex(), right[0].hex()] and ok == [True]
    assert b.hints() == hr.rows(off, P) and b.hint_stats() == stats["host"]
    b.close(); ctx.close(); s.free()
