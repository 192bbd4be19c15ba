"""k_guards_gather and k_guards_proofs alone (halo2_verifier_amd/csrc/guards_out.hip), through tests/cpp/guards_out_units.hip and
their launchers, on programmed arrays against the pure model of tests/guards_out_reference.py — exactly, in both output forms (bytes
and the object form of a resident MSM), every output between guard bands (the harness ends with status 5 on a write past one) and
with slack behind the last term that must come back untouched.

Shapes: count * T = 255, 256 and 257 (one below, at and one above the 256-thread workgroup, T = 1) and 15 x 17 = 255, 16 x 16 = 256;
T_R = 19 over 14 proofs (two workgroups) with several VK-wide bases; a channel without a VK-wide base (n_shared = 0); first > 0 and a
range that ends at n; identity points ((0, 0) -> all-zero bytes), coordinates p - 1 and scalars r - 1 (slot and VK-wide) and 0;
status words of every decoded kind, and one the decode passes through; every output alone (the others not given: untouched).

The command line of the program needs no GPU: the two checks tests/test_units_usage.py makes for the other harnesses."""
import random

import pytest

import guards_out_reference as gr
import units_harness as uh
from srs_util import P, R_MOD

PROG = "guards_out_units"
SLACK = 3
STATUS_WORDS = [0, -40, -30, -20, -10, -2]


def le32(v):
    return v.to_bytes(32, "little")


def test_usage_names_every_mode():
    r = uh.start(PROG, [])
    assert r.returncode == 2, (r.returncode, r.stderr)
    usage = [l for l in r.stderr.splitlines() if l.startswith("usage: " + PROG)]
    assert len(usage) == 1 and "gather" in usage[0].split(), r.stderr
    r = uh.start(PROG, ["no_such_mode", "a", "b"])
    assert r.returncode == 2 and "usage: " + PROG in r.stderr, (r.returncode, r.stderr)


def test_empty_input_is_too_short(tmp_path):
    empty = tmp_path / "empty.bin"
    empty.write_bytes(b"")
    out = tmp_path / "out.bin"
    r = uh.start(PROG, ["gather", empty, out])
    assert r.returncode == 2 and "input too short" in r.stderr, (r.returncode, r.stderr)
    assert not out.exists()


def _job(rnd, n, np_, n_shared, T, first, count, form, want, dead=()):
    """programmed arrays of one job with the edge values spread over them -> (header fields, arrays)"""
    kinds = [1] * min(n_shared, T // 2) + [0] * (T - min(n_shared, T // 2))
    rnd.shuffle(kinds)
    order = [(k, rnd.randrange(n_shared if k else np_)) for k in kinds]
    slot = [rnd.randrange(R_MOD) for _ in range(n * np_)]
    shared = [[rnd.randrange(R_MOD) for _ in range(n)] for _ in range(n_shared)]
    pts = [le32(rnd.randrange(P)) + le32(rnd.randrange(P)) for _ in range(n * np_ + n_shared)]
    mult = [rnd.randrange(R_MOD) for _ in range(n)]
    status = [0] * n
    for i, p in enumerate(dead):
        status[p] = STATUS_WORDS[1 + i % (len(STATUS_WORDS) - 1)]
    # the edges, inside the range: the largest scalar and coordinates, zero, the identity
    p0 = first + (1 if count > 1 and first + 1 not in dead else 0)
    if count:
        for k, (kind, idx) in enumerate(order[:4]):
            if kind:
                shared[idx][p0] = (R_MOD - 1, 0)[k % 2]
            else:
                slot[p0 * np_ + idx] = (R_MOD - 1, 0)[k % 2]
        slot[(first + count - 1) * np_ + (order[-1][1] if not order[-1][0] else 0)] = R_MOD - 1
        pts[p0 * np_ + 0] = bytes(64)
        pts[(first + count - 1) * np_ + np_ - 1] = le32(P - 1) + le32(P - 1)
        if n_shared:
            pts[n * np_ + n_shared - 1] = le32(P - 1) + le32(P - 2)
            if n_shared > 1:
                pts[n * np_] = bytes(64)
        mult[first] = R_MOD - 1
        mult[first + count - 1] = 0
    return dict(n=n, np=np_, n_shared=n_shared, T=T, first=first, count=count, form=form, want=want, order=order, slot=slot, shared=shared, pts=pts,
                mult=mult, status=status)


def _blob(j):
    b = uh.words([j["n"], j["np"], j["n_shared"], j["T"], j["first"], j["count"], SLACK, j["form"], j["want"]])
    b += uh.words([v for pair in j["order"] for v in pair])
    b += b"".join(le32(v) for v in j["slot"])
    b += b"".join(le32(v) for row in j["shared"] for v in row)
    b += b"".join(j["pts"])
    b += b"".join(le32(v) for v in j["mult"])
    b += uh.words([v & 0xffffffff for v in j["status"]])
    return b


def _check(out, j):
    terms = j["count"] * j["T"]
    sc, bs = gr.gather(j["order"], j["slot"], j["shared"], j["pts"], j["status"], j["n"], j["np"], j["first"], j["count"])
    mu, st = gr.proofs_model(j["mult"], j["status"], j["first"], j["count"])
    tag = {k: j[k] for k in ("n", "np", "n_shared", "T", "first", "count", "form", "want")}
    got = [out.take(32) for _ in range(terms + SLACK)]
    assert got[:terms] == ([le32(v) for v in sc] if j["want"] & 1 else [b"\xff" * 32] * terms), ("scalars", tag)
    assert got[terms:] == [b"\xff" * 32] * SLACK, ("scalars past the last term", tag)
    got = [out.take(64) for _ in range(terms + SLACK)]
    assert got[:terms] == (bs if j["want"] & 2 else [b"\xff" * 64] * terms), ("bases", tag)
    assert got[terms:] == [b"\xff" * 64] * SLACK, ("bases past the last term", tag)
    got = [out.take(32) for _ in range(j["count"] + SLACK)]
    assert got[:j["count"]] == ([le32(v) for v in mu] if j["want"] & 4 else [b"\xff" * 32] * j["count"]), ("multipliers", tag)
    assert got[j["count"]:] == [b"\xff" * 32] * SLACK, ("multipliers past the last proof", tag)
    got = [out.sword() for _ in range(j["count"] + SLACK)]
    assert got[:j["count"]] == (st if j["want"] & 8 else [-1] * j["count"]), ("statuses", tag)
    assert got[j["count"]:] == [-1] * SLACK, ("statuses past the last proof", tag)


@pytest.mark.gpu
@pytest.mark.parametrize("form", [0, 1], ids=["bytes", "object"])
def test_gather_is_exact(form, tmp_path):
    rnd = random.Random(2501 + form)
    jobs = []
    for count in (255, 256, 257):                                   # T = 1: around the workgroup's edge; first > 0, the range ends at n
        jobs.append(_job(rnd, count + 2, 2, 1, 1, 2, count, form, 15, dead=(5, 200)))
    jobs.append(_job(rnd, 20, 12, 6, 17, 3, 15, form, 15, dead=(4,)))            # 255
    jobs.append(_job(rnd, 16, 12, 6, 16, 0, 16, form, 15))                        # 256, the whole upload
    jobs.append(_job(rnd, 14, 12, 7, 19, 0, 14, form, 15, dead=(0, 6, 7, 8, 9, 13)))   # T_R = 19 over 14 proofs: two workgroups; every status kind
    jobs.append(_job(rnd, 9, 5, 0, 5, 1, 7, form, 15, dead=(3,)))                 # no VK-wide base at all
    jobs.append(_job(rnd, 6, 3, 2, 4, 2, 0, form, 15))                            # count = 0: nothing is written
    jobs.append(_job(rnd, 1, 1, 1, 2, 0, 1, form, 15))                            # one proof
    for want in (1, 2, 4, 8, 3, 12):                                              # outputs not given stay untouched
        jobs.append(_job(rnd, 12, 4, 3, 6, 1, 10, form, want, dead=(2,)))
    blob = uh.words([len(jobs)]) + b"".join(_blob(j) for j in jobs)
    out = uh.Cursor(uh.run(PROG, ["gather"], blob, tmp_path))
    for j in jobs:
        _check(out, j)
    out.done()
