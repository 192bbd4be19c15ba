"""Guards at the trait seam without a GPU.

  - the Python mirror (Accumulator.process_guards, Context.guards_check_each) raises before any C call on what the C side would
    index wrongly: unequal scalar / base lengths, a base that is not 64 bytes, a scalar of another length, a wrong number of draws;
  - the Python and the C++ mirror flatten the same Guards into the same counts and bytes: tests/cpp/guards_harness.cpp, a stand-alone
    program built with the address and undefined-behaviour sanitizers over the stand-in library (tests/cpp/h2v_stub.cpp +
    h2v_stub_guards.cpp, which read every array with the lengths the call's own counts give), prints a hash of every array it was
    handed; the same hashes are made here from what the Python mirror would hand over."""
import re
import struct

import pytest

import caller_harness as ch
from test_accumulator_host import _unbacked


def _guard(seed, nl, nr):
    b = lambda k, sz: bytes((seed * 31 + k * 7 + j) % 251 for j in range(sz))
    return ([b(k, 32) for k in range(nl)], [b(100 + k, 64) for k in range(nl)]), ([b(200 + k, 32) for k in range(nr)], [b(300 + k, 64) for k in range(nr)])


GUARDS = [_guard(1, 1, 19), _guard(2, 0, 3), _guard(3, 4, 0), _guard(4, 0, 0), _guard(5, 2, 7)]


def test_python_raises_before_any_c_call():
    acc, ctx = _unbacked()
    (ls, lb), (rs, rb) = GUARDS[0]
    for call in (lambda g: acc.process_guards(g), ctx.guards_check_each):
        with pytest.raises(ValueError):
            call([((ls, lb), (rs, rb[:-1]))])                         # 19 scalars, 18 bases
        with pytest.raises(ValueError):
            call([((ls + ls, lb), (rs, rb))])
        with pytest.raises(ValueError):
            call([((ls, [lb[0][:63]]), (rs, rb))])                    # a base of 63 bytes
        with pytest.raises(ValueError):
            call([((ls, [lb[0] + b"\0"]), (rs, rb))])
        with pytest.raises(ValueError):
            call([((ls, ["x" * 64]), (rs, rb))])                      # not bytes
        with pytest.raises(ValueError):
            call([(([ls[0][:31]], lb), (rs, rb))])                    # a scalar of 31 bytes
        with pytest.raises(ValueError):
            call([((ls, lb),)])                                       # one side
        with pytest.raises(ValueError):
            call([GUARDS[1], ((ls, lb), (rs, rb), (rs, rb))])
        with pytest.raises(KeyError):
            call([dict(left_scalars=ls, left_bases=lb, right_scalars=rs)])
    for rand in ([], [1], [1, 2, 3], [b"\x01" * 32]):
        with pytest.raises(ValueError):
            acc.process_guards(GUARDS[:2], rand)                      # a wrong number of draws
    with pytest.raises(ValueError):
        acc.process_guards(GUARDS[:1], [b"\x01" * 33])
    with pytest.raises(ValueError):
        acc.process_guards(GUARDS[:1], [-1])


def test_dicts_and_tuples_flatten_alike():
    from halo2_verifier_amd.verifier import _guards_args
    dicts = [dict(left_scalars=l[0], left_bases=l[1], right_scalars=r[0], right_bases=r[1], challenges=[b"c" * 32]) for l, r in GUARDS]
    a, b = _guards_args(GUARDS), _guards_args(dicts)
    assert a[0] == b[0] == 5 and [list(x) for x in a[1:3]] == [list(x) for x in b[1:3]] == [[1, 0, 4, 0, 2], [19, 3, 0, 0, 7]]
    assert a[3:] == b[3:] and [len(x) for x in a[3:]] == [32 * 7, 64 * 7, 32 * 29, 64 * 29]
    assert a[5][:32] == GUARDS[0][1][0][0] and a[5][32 * 19:32 * 20] == GUARDS[1][1][0][0]
    empty = _guards_args([])
    assert empty[0] == 0 and empty[3:] == (b"", b"", b"", b"")


def _fields(guards, rand=None):
    from halo2_verifier_amd.verifier import _guards_args
    n, lc, rc, ls, lb, rs, rb = _guards_args(guards)
    out = {"n": str(n), "left_counts": ch.fnv(struct.pack("<%dQ" % n, *list(lc)[:n])), "right_counts": ch.fnv(struct.pack("<%dQ" % n, *list(rc)[:n])),
           "ls": ch.fnv(ls), "lb": ch.fnv(lb), "rs": ch.fnv(rs), "rb": ch.fnv(rb)}
    if rand is not None:
        out["rand"] = ch.fnv(rand)
    return out


def test_cpp_and_python_mirrors_hand_over_the_same_arrays(tmp_path):
    exe = ch.build("guards_harness", tmp_path, sanitize=True, stubs=("h2v_stub", "h2v_stub_guards"))
    n, cut = len(GUARDS), 2
    rand = bytes(range(32)) * n
    guards = [dict(left_scalars=l[0], left_bases=l[1], right_scalars=r[0], right_bases=r[1]) for l, r in GUARDS]
    ch.write_dir(tmp_path, b"p" * 100, vks=[b"v" * 50], rand=rand, items_txt=ch.stand_in_items_text(n), guards_txt=ch.guards_text(guards))
    out = ch.run(exe, [tmp_path, cut], timeout=120).stdout.splitlines()
    calls = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in out if l.startswith("h2v_accumulator_process_guards ")]
    want = [_fields(GUARDS[cut:], rand[32 * cut:]), _fields(GUARDS[:cut], rand[:32 * cut]), _fields(GUARDS[cut:], rand[32 * cut:])]
    assert len(calls) == 3                                             # the refused calls never reach the library
    for got, exp in zip(calls, want):
        assert {k: got[k] for k in exp} == exp
    each = [dict(kv.split("=", 1) for kv in l.split()[1:]) for l in out if l.startswith("h2v_guards_check_each ")]
    assert len(each) == 1 and {k: each[0][k] for k in _fields(GUARDS)} == _fields(GUARDS)
    assert "refused" in out and "each 1 0 1 1 0" in out
    assert re.search(r"^h2v_accumulator_process .* n=2 ", "\n".join(out), re.M)     # the first leg of the mixed run went through process
