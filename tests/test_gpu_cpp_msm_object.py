"""The C++ mirror of the resident MSM object on the GPU (include/h2v.hpp Msm, DualMsm, Accumulator::add_msms): tests/cpp/msm_object_harness.cpp
builds a DualMsm from the Guards the library made for five proofs, scales, adds and checks, and prints verdicts and channels; they must
equal what the Python mirror computes over the same Guards, draws and factor."""
import random

import pytest

import caller_harness as ch
import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu


def test_cpp_msm_object_equals_python(tmp_path):
    import halo2_verifier_amd as h2v
    exe = ch.build("msm_object_harness", tmp_path)
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 5, seed=81, threads=4)
    rnd = random.Random(82)
    rand = [rnd.randrange(1, R_MOD) for _ in P]
    factor = rnd.randrange(2, R_MOD)
    ctx = h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))
    guards = []
    for i, (p, inst) in enumerate(zip(P, I)):
        rc, g = ctx.guard_msm(p, inst)
        assert rc == 0
        if i == 2:   # a tampered Guard: its own check fails, and with it the accumulated one
            rs = list(g["right_scalars"])
            rs[1] = ((int.from_bytes(rs[1], "little") + 1) % R_MOD).to_bytes(32, "little")
            g["right_scalars"] = rs
        guards.append(g)
    ch.write_dir(tmp_path, s.params, rand=rand, factor_bin=factor.to_bytes(32, "little"), guards_txt=ch.guards_text(guards))
    out = ch.run(exe, [tmp_path]).stdout.splitlines()
    got = {l.split()[0]: l.split()[1:] for l in out}
    # the same in Python
    D = h2v.DualMSM(ctx)
    for r, g in zip(rand, guards):
        D.scale(r)
        D.add_msm(g)
    ok, lefts, rights = h2v.dual_check_many([D])
    assert ok == [False]
    assert got["hand"] == ["0", lefts[0].hex(), rights[0].hex(), str(len(D.left)), str(len(D.right))]
    singles = []
    for g in guards:
        d = h2v.DualMSM(ctx)
        d.add_msm(g)
        singles.append(d)
    assert got["each"] == [str(int(v)) for v in h2v.dual_check_many(singles)[0]] == ["1", "1", "0", "1", "1"]
    xy, ident = h2v.eval_many([D.left, D.right, D.left])
    assert got["eval"] == [p.hex() for p in xy] + [str(int(v)) for v in ident]
    assert got["terms"] == [D.left.scalars(0, 1)[0].to_bytes(32, "little").hex(), D.right.bases(len(D.right) - 1, 1)[0].hex()]
    assert got["clone"] == [str(len(D.left) + 1), str(len(D.left))]
    acc = h2v.Accumulator(ctx)
    acc.add_msms(D)
    acc.add_msms((D.left, None))
    okf, l, r = acc.finalize()
    assert got["acc"] == [str(int(okf)), l.hex(), r.hex()]
    E = D.left.clone(), D.right.clone()
    E[0].scale(factor); E[1].scale(factor)
    ok2, l2, r2 = h2v.dual_check_many([h2v.DualMSM(ctx, *E)])
    assert got["scaled"] == [str(int(ok2[0])), l2[0].hex(), r2[0].hex()]
    assert got["empty"] == ["0", "0"]
    n0 = len(guards[0]["left_scalars"])
    assert got["moved"] == [str(n0), str(n0), str(len(guards[0]["right_scalars"]))]
    assert got["refused"] == ["8"]
    ctx.close()
    s.free()
