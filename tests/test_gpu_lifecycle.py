"""The life of a staged batch: upload -> launch -> finish, each stage committed only when its call succeeded.  After a failed upload
the batch holds nothing — launch, finish, finish_groups, recheck and fold_check_enqueue are refused until an upload succeeds, and
that upload gives bit for bit what a fresh batch gives (no verdict, statuses or accumulators of the earlier upload can come back).
The one-shot calls share the context's scratch batch; a call that failed must leave it fit for the next."""
import random

import pytest

import circuits
from circuits import R_MOD

pytestmark = pytest.mark.gpu

N = 8


@pytest.fixture(scope="module")
def pool():
    s = circuits.setup_vector_mul(8, 8)
    P, I = circuits.prove_vector_mul_batch(s, 4 * N, seed=2718, threads=16)
    yield s, P, I
    s.free()


def _ctx(s):
    import halo2_verifier_amd as h2v
    return h2v.Context(h2v.ParamsKZG(s.params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(s.vk, h2v.SerdeFormat.RawBytes))


def _flat(P, I):
    return b"".join(P), b"".join(b"".join(col) for i in I for col in i)


def _draws(n, seed):
    rnd = random.Random(seed)
    return [rnd.randrange(1, R_MOD) for _ in range(n)]


def _rand_bytes(rand):
    return b"".join(r.to_bytes(32, "little") for r in rand)


def _tampered(P, I):
    """(P, I) with proof 0's first public input changed: every proof decodes, only the pairing rejects the batch."""
    I = [[list(c) for c in inst] for inst in I]
    I[0][0][0] = ((int.from_bytes(I[0][0][0], "little") + 1) % R_MOD).to_bytes(32, "little")
    return list(P), I


def _fresh(ctx, flat, inst, rb):
    import halo2_verifier_amd as h2v
    b = h2v.Batch(ctx, N, 8)
    b.upload(flat, 1024, inst, [8], rb)
    b.launch()
    out = b.finish()
    b.close()
    return out


def _assert_refused_until_upload(b, record):
    import halo2_verifier_amd as h2v
    calls = [("launch", b.launch), ("finish", b.finish), ("finish_groups", b.finish_groups), ("recheck", lambda: b.recheck([(0, 1)])),
             ("fold_check_enqueue", lambda: b.fold_check_enqueue(record.data_ptr(), 1))]
    for name, call in calls:
        with pytest.raises(h2v.H2VError) as e:
            call()
        assert e.value.code == -16, name


def _valid_record(ctx, P, I, rb):
    """A well-formed accumulator record in device memory (another batch's export), for the fold that must be refused."""
    import torch
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import distributed as h2d
    rec = torch.zeros(h2d.ACC_BYTES, dtype=torch.uint8, device="cuda:0")
    other = h2v.Batch(ctx, N, 8)
    flat, inst = _flat(P, I)
    other.upload(flat, 1024, inst, [8], rb)
    other.launch(with_pairing=False)
    other.export_accumulators(rec.data_ptr())
    other.finish()
    other.close()
    return rec


@pytest.mark.parametrize("staged", ["upload", "upload_launch"])
def test_a_failed_upload_leaves_nothing_to_launch(pool, staged):
    import halo2_verifier_amd as h2v
    s, P0, I0 = pool
    ctx = _ctx(s)
    P, I = P0[:N], I0[:N]
    rb = _rand_bytes(_draws(N, 31))
    record = _valid_record(ctx, P0[N:2 * N], I0[N:2 * N], rb)
    b = h2v.Batch(ctx, N, 8)
    flat, inst = _flat(P, I)

    def run(flat, inst, rb):
        if staged == "upload":
            b.upload(flat, 1024, inst, [8], rb)
            b.launch()
        else:
            b.upload_launch(flat, 1024, inst, [8], rb)
        return b.finish()

    first = run(flat, inst, rb)
    assert first[0] is True and first[1] == [0] * N
    Pt, It = _tampered(P, I)
    tflat, tinst = _flat(Pt, It)
    with pytest.raises(h2v.H2VError) as e:   # a draw that is not a canonical scalar
        run(tflat, tinst, b"\xff" * 32 + rb[32:])
    assert e.value.code == -16
    _assert_refused_until_upload(b, record)
    got = run(tflat, tinst, rb)
    assert got == _fresh(ctx, tflat, tinst, rb)
    assert got[0] is False and got[1] == [0] * N
    b.close()
    ctx.close()


def test_set_groups_refuses_the_finished_launch_until_the_next_upload(pool):
    import halo2_verifier_amd as h2v
    s, P0, I0 = pool
    ctx = _ctx(s)
    P, I = P0[:N], I0[:N]
    rb = _rand_bytes(_draws(N, 32))
    flat, inst = _flat(P, I)
    b = h2v.Batch(ctx, N, 8)
    b.upload(flat, 1024, inst, [8], rb)
    b.launch()
    first = b.finish_groups()
    assert first[0] == [True]
    b.set_groups(2)
    for call in (b.finish_groups, b.launch, lambda: b.recheck([(0, 1)])):
        with pytest.raises(h2v.H2VError):
            call()
    b.upload(flat, 1024, inst, [8], rb)
    b.launch()
    got = b.finish_groups()
    g = h2v.Batch(ctx, N, 8, groups=2)
    g.upload(flat, 1024, inst, [8], rb)
    g.launch()
    assert got == g.finish_groups()
    assert got[0] == [True, True]
    g.close()
    b.close()
    ctx.close()


def test_the_scratch_batch_survives_a_failed_one_shot_call(pool):
    import halo2_verifier_amd as h2v
    s, P0, I0 = pool
    ctx = _ctx(s)
    rand = _draws(N, 33)
    with pytest.raises(h2v.H2VError) as e:
        ctx.verify_batch(P0[:N], I0[:N], [R_MOD] + rand[1:])
    assert e.value.code == -16
    P, I = _tampered(P0[2 * N:3 * N], I0[2 * N:3 * N])
    got = (ctx.verify_batch(P, I, rand), ctx.verify_each(P, I), ctx.verify_batch_identify(P, I, rand), ctx.guard_msm(P[1], I[1]),
           ctx.verify_batch(P0[3 * N:], I0[3 * N:], rand))
    fresh = _ctx(s)
    exp = (fresh.verify_batch(P, I, rand), fresh.verify_each(P, I), fresh.verify_batch_identify(P, I, rand), fresh.guard_msm(P[1], I[1]),
           fresh.verify_batch(P0[3 * N:], I0[3 * N:], rand))
    assert got == exp
    assert got[0][0] is False and got[1] == [h2v.PlonkError.ConstraintSystemFailure] + [0] * (N - 1)
    assert got[2][1] == got[1] and got[3][0] == 0 and got[4][0] is True
    fresh.close()
    ctx.close()
