"""Hint rows on the host (include/h2v_hint_rows.h): where its four entry points are declared, exported and bound, the fields the
decompression stage gained for its miss list, the C++ mirror's header, the refusals that need no device and the Python refusals that
need no library, and the arithmetic of the counters against tests/hints_reference.py.  The kernels are
tests/test_gpu_hints_list_units.py's, the entry points on a GPU tests/test_gpu_hinted_calls.py's."""
import ctypes
import os
import random
import re
import subprocess
import types

import pytest

import caller_harness
import hints_reference as hr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = sorted(["h2v_batch_set_hint_rows", "h2v_verify_batch_keys_hinted", "h2v_verify_batches_hinted", "h2v_accumulator_process_hinted"])


@pytest.fixture(scope="module")
def lib():
    import halo2_verifier_amd as h2v
    if not os.path.exists(h2v.lib_path()):
        subprocess.check_call(["make", "-j", "4", "-C", os.path.join(ROOT, "halo2_verifier_amd", "csrc")])
    lib = ctypes.CDLL(h2v.lib_path())
    lib.h2v_last_error.restype = ctypes.c_char_p
    return lib


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(h2v_[a-z0-9_]+)\s*\(", text)))


# ------------------------------------------------------------------ bindings
def test_symbols_are_exported_declared_in_their_own_header_and_bound(lib):
    from halo2_verifier_amd import _lib, hints
    assert _declared("h2v_hint_rows.h") == NAMES
    assert sorted(hints.ROW_SIGNATURES) == NAMES and not set(NAMES) & set(hints.SIGNATURES) and not set(NAMES) & set(_lib.SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert all(re.search(r" T %s$" % n, out, re.M) for n in NAMES)
    for other in ("h2v.h", "h2v_draws.h", "h2v_guards.h", "h2v_hints.h"):
        assert not set(NAMES) & set(_declared(other)), other
    bound = hints._library()
    assert all(getattr(bound, n).argtypes == hints.ROW_SIGNATURES[n][1] for n in NAMES)
    rs = open(os.path.join(ROOT, "integration", "rust", "hint_rows.rs")).read()
    assert sorted(set(re.findall(r"pub fn (h2v_[a-z0-9_]+)\s*\(", rs))) == NAMES
    # each _hinted call is its unhinted form plus hint_rows after proof_lens and hint_stats last
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "h2v_hint_rows.h")).read(), flags=re.S)
    plain = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "h2v.h")).read(), flags=re.S)
    params = lambda src, name: [" ".join(p.split()) for p in re.search(r"\b%s\s*\(([^)]*)\)" % name, src).group(1).split(",")]
    for name in ("h2v_verify_batch_keys", "h2v_verify_batches", "h2v_accumulator_process"):
        base, got = params(plain, name), params(text, name + "_hinted")
        at = base.index("const size_t* proof_lens") + 1
        assert got == base[:at] + ["const uint8_t* const* hint_rows"] + base[at:] + ["size_t hint_stats[3]"], name
    head = open(os.path.join(ROOT, "include", "h2v_hints.h")).read()
    assert "Out of its reach" not in head and "h2v_hint_rows.h" in head


def test_the_stage_takes_a_miss_list_last_and_null_by_default():
    text = open(os.path.join(ROOT, "halo2_verifier_amd", "csrc", "batch.h")).read()
    body = re.search(r"struct StageArgs \{(.*?)\n\};", text, re.S).group(1)
    fields = re.findall(r"^\s+(?:const )?\w[\w ]*\*+ ?(\w+) = nullptr;", body, re.M)
    assert fields == ["hint_misses", "hints", "miss_list", "miss_list_count"]
    kernels = open(os.path.join(ROOT, "halo2_verifier_amd", "csrc", "verify_kernels.hip")).read()
    # one hinted kernel, always with the list: no instantiation without one
    assert "k_decompress_misses" in kernels and "k_decompress_hinted(" in kernels and "k_decompress_hinted<" not in kernels and "LISTED" not in kernels


def test_null_arguments_are_refused_before_any_device_work(lib):
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    rows = (ctypes.c_char_p * 1)(b"\0" * 32)
    assert lib.h2v_batch_set_hint_rows(vp(None), sz(1), rows) == -16 and b"h2v_batch_set_hint_rows" in lib.h2v_last_error()
    stats = (sz * 3)(7, 7, 7)
    assert lib.h2v_verify_batch_keys_hinted(None, sz(1), None, sz(1), None, None, rows, None, None, None, None, None, None, None, None, stats) == -16
    assert b"h2v_verify_batch_keys_hinted" in lib.h2v_last_error()
    assert lib.h2v_verify_batches_hinted(vp(None), sz(1), None, None, None, rows, None, sz(0), None, None, None, None, None, None, stats) == -16
    assert b"h2v_verify_batches_hinted" in lib.h2v_last_error()
    assert lib.h2v_accumulator_process_hinted(vp(None), None, sz(1), None, sz(0), None, None, rows, None, None, None, None, None, None, stats) == -16
    assert b"h2v_accumulator_process_hinted" in lib.h2v_last_error()
    assert list(stats) == [7, 7, 7]                                          # a call that fails writes no counters


def test_cpp_mirror_header_compiles(tmp_path):
    src = tmp_path / "use_hint_rows.cpp"
    src.write_text('#include "h2v_hints.hpp"\n'
                   "int main() {\n"
                   "    try {\n"
                   "        h2v::Context* c = nullptr;\n"
                   "        std::vector<h2v::hints::Item> items;\n"
                   "        h2v::hints::Result r = h2v::hints::verify_batch_keys({c}, items);\n"
                   "        h2v::hints::Stats s;\n"
                   "        auto rs = h2v::hints::verify_batches(*c, {items}, h2v::Bytes(), &s);\n"
                   "        h2v::Accumulator acc(*c);\n"
                   "        auto st = h2v::hints::process(acc, {c}, items, h2v::Bytes(), &s);\n"
                   "        h2v::hints::set_rows(nullptr, {h2v::Bytes()}, 3);\n"
                   "        return (int)(r.statuses.size() + rs.size() + st.size() + s.points);\n"
                   "    } catch (const h2v::Failure&) { return 0; }\n"
                   "}\n")
    caller_harness.check_syntax(src)
    caller_harness.check_syntax("hinted_calls.cpp")


# ------------------------------------------------------------------ Python-side refusals, without a library call
def _no_library(monkeypatch):
    from halo2_verifier_amd import hints

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hints, "_library", no_library)


def _bare_batch(n=4, n_points=3):
    from halo2_verifier_amd import verifier
    b = verifier.Batch.__new__(verifier.Batch)
    b.n, b._keep, b._hint_points = n, None, n_points
    b.ctx = types.SimpleNamespace(device=0)
    return b


def test_batch_set_hint_rows_refuses_without_the_library(monkeypatch):
    _no_library(monkeypatch)
    b = _bare_batch()                                 # rows of 96 bytes, 4 proofs
    row = b"\1" * 96
    for rows in ([row] * 3, [row] * 5, []):
        with pytest.raises(ValueError, match="4 proofs need 4 hint rows"):
            b.set_hint_rows(rows)
    for bad in (b"\1" * 95, b"\1" * 97, b""):
        with pytest.raises(ValueError, match="hint row 2 must hold n_points \\* 32 = 96 bytes"):
            b.set_hint_rows([row, None, bad, row])
    for bad in ("x" * 96, 5, [row]):
        with pytest.raises(TypeError, match="hint row 1 must be bytes or None"):
            b.set_hint_rows([None, bad, row, row])
    for bad in (row * 4, 7, "rows"):
        with pytest.raises(TypeError, match="sequence"):
            b.set_hint_rows(bad)


def test_the_one_shot_mirrors_refuse_without_the_library(monkeypatch):
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import distributed, verifier
    _no_library(monkeypatch)

    def fake_ctx(n_points):
        c = verifier.Context.__new__(verifier.Context)
        c._hint_points, c._h = n_points, ctypes.c_void_p()      # (closed: __del__ has nothing to destroy)
        return c
    c3, c5 = fake_ctx(3), fake_ctx(5)
    acc = verifier.Accumulator.__new__(verifier.Accumulator)
    acc._h = ctypes.c_void_p()
    proofs, inst = [b"p" * 40] * 3, [[[b"\0" * 32]]] * 3
    r3, r5 = b"\2" * 96, b"\2" * 160
    calls = [lambda h: c3.verify_batch(proofs, inst, None, hints=h),
             lambda h: h2v.verify_batch_keys([c3], [0, 0, 0], proofs, inst, None, hints=h),
             lambda h: c3.verify_batches([(proofs[:1], inst[:1]), (proofs[1:], inst[1:])], None, hints=h),
             lambda h: acc.process(c3, None, proofs, inst, None, hints=h)]
    for call in calls:
        with pytest.raises(ValueError, match="3 proofs need 3 hint rows"):
            call([r3, None])
        with pytest.raises(ValueError, match="hint row 2 must hold n_points \\* 32 = 96 bytes"):
            call([r3, None, r5])
        with pytest.raises(TypeError, match="hint row 0 must be bytes or None"):
            call(["x" * 96, None, None])
        with pytest.raises(TypeError, match="sequence"):
            call(r3 * 3)
    # a row is as long as ITS proof's key asks
    with pytest.raises(ValueError, match="hint row 1 must hold n_points \\* 32 = 160 bytes"):
        h2v.verify_batch_keys([c3, c5], [0, 1, 0], proofs, inst, None, hints=[r3, r3, r3])
    with pytest.raises(ValueError, match="a seeded batch takes no hints"):
        c3.verify_batch(proofs, inst, None, seed=(([], []), ([], [])), hints=[None] * 3)
    with pytest.raises(TypeError, match="one row of bytes"):
        h2v.verify_proof(None, None, h2v.AccumulatorStrategy(None), inst[0], proofs[0], hints=[r3])
    for call in (lambda h: distributed.verify_batch_sharded_local(c3, proofs, inst, None, world=2, hints=h),
                 lambda h: distributed.verify_batch_sharded(c3, proofs, inst, None, hints=h)):
        with pytest.raises(ValueError, match="3 proofs need 3 hint rows"):
            call([r3] * 4)
        with pytest.raises(TypeError, match="sequence"):
            call(r3)


def test_a_sharded_rank_stages_its_own_slice():
    """ShardedBatch hands rows to its batch; the sharded calls cut [lo, hi) for every rank (a stand-in batch records what it is given)"""
    from halo2_verifier_amd import distributed
    seen = []

    class Stand:
        n = 0
        def __init__(self, *a): pass
        def upload(self, flat, plen, iflat, lens, tail): self.n = len(flat) // plen
        def set_hint_rows(self, rows): seen.append(("rows", list(rows)))
        def set_hints(self, y32): seen.append(("flat", y32))
        def close(self): pass
    sb = distributed.ShardedBatch(None, 4, 1, batch_factory=lambda c, n, mi, st, g: Stand(), device="cpu")
    sb.set_hint_rows([b"a", None])
    sb.set_hints(b"bb")
    assert seen == [("rows", [b"a", None]), ("flat", b"bb")]
    rows = [bytes([i]) * 96 if i % 2 else None for i in range(7)]
    for world in (1, 2, 3, 7, 9):
        cuts = [distributed.shard_bounds(7, world, r) for r in range(world)]
        assert [x for lo, hi in cuts for x in distributed._hint_rows(rows, 7)[lo:hi]] == rows


# ------------------------------------------------------------------ the counters' arithmetic
def test_expected_stats_is_the_reference_count():
    from halo2_verifier_amd import hints
    rnd = random.Random(9)
    np_of = [3, 5, 3, 3, 5, 4, 3, 5]
    pts = [[hr.random_point(rnd) for _ in range(k)] for k in np_of]
    pts[2][1] = hr.encode(hr.P + 1, 0)                                         # an undecodable point under a row
    pts[3][0] = hr.encode(hr.non_residue_x(77), 1)                             # and one in a proof without a row
    right = [hr.hint_set("right", p) for p in pts]
    rows = [right[0], None, right[2], None, hr.hint_set("other_root", pts[4]), hr.hint_set("even_lanes", pts[5]), None, right[7]]
    missed = [0 if r is None else hr.count_misses(p, r) for p, r in zip(pts, rows)]
    assert missed == [0, 0, 1, 0, 5, 2, 0, 0]
    want = (sum(np_of), 3 + 3 + 5 + 4 + 5, 8)
    assert hints.expected_stats(np_of, rows, missed) == want
    # what the device counts: every point of a proof without a row misses (a zero hint); the library subtracts them again
    staged = [r if r is not None else bytes(32 * k) for r, k in zip(rows, np_of)]
    device_missed = sum(hr.count_misses(p, r) for p, r in zip(pts, staged))
    null_points = sum(k for k, r in zip(np_of, rows) if r is None)
    assert device_missed == want[2] + null_points and (want[0], want[0] - null_points, device_missed - null_points) == want
    assert hints.expected_stats(np_of, [None] * 8, [0] * 8) == (sum(np_of), 0, 0)
    assert hints.expected_stats([], [], []) == (0, 0, 0)
