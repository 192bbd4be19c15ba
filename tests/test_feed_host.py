"""The enqueued feed of a resident accumulator (include/h2v_feed.h), without a GPU: where its three entry points are declared, bound
and exported, the Python mirror's own refusals, and the host bookkeeping of pending feeds as tests/feed_reference.py models it.
The device side is tests/test_gpu_feed.py's."""
import ctypes
import os
import re
import subprocess

import pytest

import caller_harness
import feed_reference as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["h2v_accumulator_feed_batch", "h2v_accumulator_pending", "h2v_accumulator_settle"]


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(h2v_[a-z0-9_]+)\s*\(", text)))


@pytest.fixture(scope="module")
def lib_path():
    import halo2_verifier_amd as h2v
    if not os.path.exists(h2v.lib_path()):
        subprocess.check_call(["make", "-j", "4", "-C", os.path.join(ROOT, "halo2_verifier_amd", "csrc"), "build/libh2v_amd.so"])
    return h2v.lib_path()


def test_header_table_and_rust_name_the_same_functions_and_constant():
    from halo2_verifier_amd import _lib, feed
    assert _declared("h2v_feed.h") == NAMES
    assert sorted(feed.SIGNATURES) == NAMES
    rs = open(os.path.join(ROOT, "integration", "rust", "feed.rs")).read()
    assert sorted(set(re.findall(r"pub fn (h2v_[a-z0-9_]+)\s*\(", rs))) == NAMES
    header = open(os.path.join(ROOT, "include", "h2v_feed.h")).read()
    limit = int(re.search(r"#define H2V_FEED_MAX_PENDING (\d+)", header).group(1))
    assert limit == 64 == feed.FEED_MAX_PENDING == fr.FEED_MAX_PENDING
    assert limit == int(re.search(r"pub const H2V_FEED_MAX_PENDING: usize = (\d+);", rs).group(1))
    # argument counts: the header's parameter lists against the ctypes table
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for name in NAMES:
        params = re.search(r"\b%s\s*\(([^)]*)\)" % name, text).group(1)
        assert len(params.split(",")) == len(feed.SIGNATURES[name][1]), name
        assert feed.SIGNATURES[name][0] is ctypes.c_int
    # h2v.h, its table and ffi.rs stay the binding of h2v.h alone
    assert not set(NAMES) & set(_declared("h2v.h")) and not set(NAMES) & set(_lib.SIGNATURES)
    assert not any(n in open(os.path.join(ROOT, "include", "h2v.h")).read() for n in NAMES)
    assert not any(n in open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read() for n in NAMES)


def test_the_library_exports_all_three(lib_path):
    out = subprocess.run(["nm", "-D", "--defined-only", lib_path], capture_output=True, text=True, check=True).stdout
    assert all(re.search(r" T %s$" % n, out, re.M) for n in NAMES)
    lib = ctypes.CDLL(lib_path)
    assert all(hasattr(lib, n) for n in NAMES)
    # null arguments are refused before anything else, without a device
    lib.h2v_last_error.restype = ctypes.c_char_p
    for n in NAMES:
        getattr(lib, n).restype = ctypes.c_int
    assert lib.h2v_accumulator_feed_batch(None, None) == fr.BAD_ARGUMENT and b"null" in lib.h2v_last_error()
    assert lib.h2v_accumulator_pending(None, None, None) == fr.BAD_ARGUMENT
    assert lib.h2v_accumulator_settle(None, ctypes.c_size_t(0), None, None, None, None) == fr.BAD_ARGUMENT


def test_cpp_mirror_header_compiles(tmp_path):
    src = tmp_path / "use_feed.cpp"
    src.write_text('#include "h2v_feed.hpp"\n'
                   "int main() {\n"
                   "    h2v_accumulator* a = nullptr; h2v_batch* b = nullptr;\n"
                   "    if (a) {\n"
                   "        h2v::feed::feed_batch(a, b);\n"
                   "        h2v::feed::Pending p = h2v::feed::pending(a);\n"
                   "        std::vector<h2v::feed::Report> r = h2v::feed::settle(a);\n"
                   "        return (int)(p.unsettled + p.unreported + r.size());\n"
                   "    }\n"
                   "    return H2V_FEED_MAX_PENDING == 64 ? 0 : 1;\n"
                   "}\n")
    caller_harness.check_syntax(src)


def test_python_side_refusals():
    """a non-Batch argument, keep_inputs and a closed batch or accumulator are refused before the library is asked"""
    from halo2_verifier_amd import verifier
    acc = verifier.Accumulator.__new__(verifier.Accumulator)
    acc._h, acc._keep_inputs, acc._inputs, acc._fed_groups, acc._feed_reports = ctypes.c_void_p(1), False, [], [], []
    batch = verifier.Batch.__new__(verifier.Batch)
    batch._h = ctypes.c_void_p()          # closed
    with pytest.raises(TypeError, match="Batch"):
        acc.feed(object())
    with pytest.raises(TypeError, match="Batch"):
        acc.feed(None)
    with pytest.raises(ValueError, match="closed"):
        acc.feed(batch)
    keeper = verifier.Accumulator.__new__(verifier.Accumulator)
    keeper._h, keeper._keep_inputs, keeper._inputs, keeper._fed_groups, keeper._feed_reports = ctypes.c_void_p(1), True, [], [], []
    batch._h = ctypes.c_void_p(1)
    with pytest.raises(ValueError, match="Batch.identify"):
        keeper.feed(batch)
    closed = verifier.Accumulator.__new__(verifier.Accumulator)
    closed._h, closed._fed_groups, closed._feed_reports = ctypes.c_void_p(), [], []
    with pytest.raises(ValueError, match="closed"):
        closed.feed(batch)
    with pytest.raises(ValueError, match="closed"):
        closed.settle()
    with pytest.raises(ValueError, match="closed"):
        closed.pending
    assert acc._fed_groups == [] and keeper._fed_groups == []
    for o in (acc, keeper, closed):       # (nothing to destroy)
        o._h = ctypes.c_void_p()


def test_model_feed_then_settle_is_process_batch():
    fed, ref = fr.Model(capacity=12), fr.Model(capacity=12)
    for sizes, failed in [([4, 4], [0, 1]), ([1, 5, 2], [0, 0, 0]), ([7], [2])]:
        fed.feed(sizes)
        ref.process_batch(sizes, failed)
    assert fed.pending == (3, 3) and fed.legs() == [(0, 0)] and fed.n_proofs == 0     # the host knows nothing before settle
    assert fed.free == [11, 10, 9, 8, 7]                                               # ... but the slots are taken
    reports = fed.settle([(0, [0, 1]), (0, [0, 0, 0]), (0, [2])])
    assert reports == [(0, 8, 1), (0, 8, 0), (0, 7, 2)]
    assert fed.entries == ref.entries and fed.free == ref.free
    assert (fed.n_proofs, fed.n_failed) == (ref.n_proofs, ref.n_failed) == (23, 3)
    assert fed.pending == (0, 0) and fed.settle() == []


def test_model_a_refused_feed_between_two_good_ones():
    m = fr.Model(capacity=8)
    m.feed([2, 3])                      # slots 1, 2
    m.feed([4, 4, 1])                   # slots 3, 4, 5: dropped on the device
    m.feed([6])                         # slot 6
    assert m.free == [7]
    with pytest.raises(fr.Refused) as e:
        m.feed([1, 1])                  # 1 entry + 6 pending legs + 2 > 8
    assert e.value.code == fr.UNSUPPORTED and m.pending == (3, 3) and m.free == [7]
    m.commit([(0, [0, 0]), (fr.BAD_ARGUMENT, None), (0, [1])])      # an implicit settle: the reports stay
    assert m.pending == (0, 3)
    assert m.entries == [(0, 0, 0), (1, 2, 0), (2, 3, 0), (6, 6, 1)]
    assert m.free == [7, 5, 4, 3]                                   # the dropped feed's slots are free again, lowest first
    assert (m.n_proofs, m.n_failed) == (5 + 9 + 6, 0 + 9 + 1)       # the dropped feed: processed AND failed
    assert m.settle() == [(0, 5, 0), (fr.BAD_ARGUMENT, 9, 9), (0, 6, 1)]
    # the next feed takes the lowest free slots, as a process_batch would
    m.feed([1, 1, 1, 1])
    assert m.settle([(0, [0] * 4)]) == [(0, 4, 0)]
    assert [slot for slot, _, _ in m.entries[4:]] == [3, 4, 5, 7] and m.free == []
    with pytest.raises(fr.Refused):
        m.feed([1])
    # drop_legs afterwards: counters are the kept entries' — the dropped feed's 9 failed proofs belong to no entry and leave with it
    m.drop([3])
    assert m.legs() == [(0, 0), (2, 0), (3, 0), (1, 0), (1, 0), (1, 0), (1, 0)] and (m.n_proofs, m.n_failed) == (9, 0)


def test_model_the_65th_unreported_feed_and_journal_off():
    m = fr.Model()                      # journal off: no slots, no entries, only counters and reports
    for _ in range(fr.FEED_MAX_PENDING):
        m.feed([3])
    with pytest.raises(fr.Refused) as e:
        m.feed([3])
    assert e.value.code == fr.UNSUPPORTED
    m.commit([(0, [0])] * 64)           # settled on the way, not reported: still refused
    with pytest.raises(fr.Refused):
        m.feed([3])
    assert len(m.settle()) == 64 and m.n_proofs == 192 and m.entries == []
    m.feed([3])
    m.feed([])                          # no proofs: nothing enqueued, no report
    assert m.pending == (1, 1)
