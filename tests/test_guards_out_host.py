"""Every proof's Guard out of a launch, on the host: where the four entry points of include/h2v_guards.h are declared, exported and
bound, the C++ mirror's header, and the Python refusals that need no library (ranges and lengths).  The kernel is
tests/test_gpu_guards_out_units.py's, the entry points on a GPU tests/test_gpu_guards_out.py's."""
import ctypes
import os
import re
import subprocess

import pytest

import caller_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["h2v_batch_guard_shape", "h2v_batch_guards", "h2v_batch_guards_append", "h2v_batch_guards_device"]


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


def test_symbols_are_exported_declared_in_their_own_header_and_bound(lib):
    from halo2_verifier_amd import _lib, guards
    assert _declared("h2v_guards.h") == NAMES
    assert all(hasattr(lib, n) for n in NAMES)
    assert not set(NAMES) & set(_declared("h2v.h")) and not set(NAMES) & set(_lib.SIGNATURES)
    assert not set(NAMES) & set(_declared("h2v_draws.h"))
    assert sorted(guards.SIGNATURES) == NAMES
    rs = open(os.path.join(ROOT, "integration", "rust", "guards.rs")).read()
    assert sorted(set(re.findall(r"pub fn (h2v_[a-z0-9_]+)\s*\(", rs))) == NAMES
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert all(re.search(r" T %s$" % n, out, re.M) for n in NAMES)
    text = open(os.path.join(ROOT, "include", "h2v_guards.h")).read()
    assert '#include "h2v.h"' in text and "one thread at a time" in text and "sum-equal" in text


def test_null_batch_is_refused_before_any_device_work(lib):
    """no context, no device: every entry point refuses a null batch with BAD_ARGUMENT"""
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    n = sz(7)
    assert lib.h2v_batch_guard_shape(vp(None), ctypes.byref(n), ctypes.byref(n)) == -16 and b"h2v_batch_guard_shape" in lib.h2v_last_error()
    assert n.value == 7
    assert lib.h2v_batch_guards_device(vp(None), sz(0), sz(1), *[vp(None)] * 6) == -16 and b"h2v_batch_guards_device" in lib.h2v_last_error()
    assert lib.h2v_batch_guards(vp(None), sz(0), sz(1), *[vp(None)] * 6) == -16
    assert lib.h2v_batch_guards_append(vp(None), sz(0), sz(1), vp(None), vp(None), ctypes.byref(n)) == -16 and n.value == 7


def _bare_batch(n):
    from halo2_verifier_amd import verifier
    b = verifier.Batch.__new__(verifier.Batch)
    b.n = n
    return b


def test_python_refuses_ranges_outside_the_upload_without_the_library(monkeypatch):
    from halo2_verifier_amd import guards

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(guards, "_library", no_library)
    b = _bare_batch(10)
    for call in (lambda f, c: b.guards(f, c), lambda f, c: b.guards_into(f, c, status=4096), lambda f, c: b.guards_append(None, None, f, c)):
        for first, count in ((11, 0), (0, 11), (4, 7), (10, 1), (-1, 2), (0, -1), (2**64, 0)):
            with pytest.raises(ValueError):
                call(first, count)
        for first, count in ((1.5, 1), (0, "2"), (True, 1)):
            with pytest.raises(TypeError):
                call(first, count)
    assert b.guards(10, None) == [] and b.guards(3, 0) == []        # an empty range: nothing to ask the library
    with pytest.raises(ValueError, match="no output"):
        b.guards_into(0, 1)
    with pytest.raises(ValueError, match="16-byte"):
        b.guards_into(0, 1, mult=4104)
    with pytest.raises(TypeError):
        b.guards_into(0, 1, mult=4096.0)
    with pytest.raises(TypeError, match="MSMKZG"):
        b.guards_append(object(), None)
    with pytest.raises(TypeError, match="MSMKZG"):
        b.guards_append(None, b"")


def test_python_checks_tensor_lengths_against_the_shape(monkeypatch):
    """every length the C side indexes is validated in Python first: a tensor of the wrong size, dtype or device never reaches it"""
    from halo2_verifier_amd import guards

    class Dev:
        type, index = "cuda", 0

    class Fake:
        def __init__(self, numel, dtype="torch.uint8", index=0):
            self.dtype, self.shape, self.device = dtype, (numel,), Dev()
            self.device.index = index
        def stride(self): return (1,)
        def data_ptr(self): return 4096

    class Ctx:
        device = 0
    b = _bare_batch(10)
    b.ctx = Ctx()
    monkeypatch.setattr(guards, "guard_shape", lambda batch: (1, 19))

    def no_call(*a):
        raise AssertionError("the library was reached")
    monkeypatch.setattr(guards, "guards_device", no_call)
    assert guards.output_sizes(4, (1, 19)) == (128, 256, 2432, 4864, 128, 16)
    with pytest.raises(ValueError, match="2432 elements"):
        b.guards_into(2, 4, right_scalars=Fake(2431))
    with pytest.raises(ValueError, match="256 elements"):
        b.guards_into(2, 4, left_bases=Fake(128))
    with pytest.raises(ValueError, match="4 elements"):
        b.guards_into(2, 4, status=Fake(16, "torch.int32"))
    with pytest.raises(TypeError, match="int32"):
        b.guards_into(2, 4, status=Fake(4, "torch.int64"))
    with pytest.raises(TypeError, match="uint8"):
        b.guards_into(2, 4, mult=Fake(128, "torch.int32"))
    with pytest.raises(ValueError, match="context's device"):
        b.guards_into(2, 4, mult=Fake(128, index=1))
    with pytest.raises(ValueError, match="2\\^31"):
        guards.output_sizes(1 << 27, (1, 19))


def test_cpp_mirror_header_compiles(tmp_path):
    src = tmp_path / "use_guards.cpp"
    src.write_text('#include "h2v_guards.hpp"\n'
                   "int main() {\n"
                   "    h2v_batch* b = nullptr;\n"
                   "    try {\n"
                   "        h2v::guards::Shape s = h2v::guards::shape(b);\n"
                   "        h2v::guards::HostGuards g = h2v::guards::to_host(b, 0, 1);\n"
                   "        h2v::Guard one = h2v::guards::guard_of(g, 0);\n"
                   "        h2v::guards::DeviceGuards d;\n"
                   "        h2v::guards::to_device(b, 0, 0, d);\n"
                   "        size_t failed = h2v::guards::append(b, 0, 0, nullptr, nullptr);\n"
                   "        return (int)(s.left_terms + one.left_scalars.size() + failed);\n"
                   "    } catch (const h2v::Failure&) { return 0; }\n"
                   "}\n")
    caller_harness.check_syntax(src)
