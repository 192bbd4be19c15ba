"""Point hints on the host (include/h2v_hints.h): where its seven entry points are declared, exported and bound, the C++ mirror's
header, h2v_hints_from_points — host code, no device — against tests/hints_reference.decode, and the Python refusals that need no
library.  The kernel is tests/test_gpu_hints_list_units.py's, the entry points on a GPU tests/test_gpu_hints.py's."""
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
NAMES = sorted(["h2v_hints_point_offsets", "h2v_hints_from_points", "h2v_batch_set_hints", "h2v_batch_set_hints_device", "h2v_batch_hints",
                "h2v_batch_hints_device", "h2v_batch_hint_stats"])


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
    assert _declared("h2v_hints.h") == NAMES
    assert sorted(hints.SIGNATURES) == NAMES
    assert all(hasattr(lib, n) for n in NAMES)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert all(re.search(r" T %s$" % n, out, re.M) for n in NAMES)
    for other in ("h2v.h", "h2v_draws.h", "h2v_guards.h"):
        assert not set(NAMES) & set(_declared(other)), other
    assert not set(NAMES) & set(_lib.SIGNATURES)
    rs = open(os.path.join(ROOT, "integration", "rust", "hints.rs")).read()
    assert sorted(set(re.findall(r"pub fn (h2v_[a-z0-9_]+)\s*\(", rs))) == NAMES
    text = open(os.path.join(ROOT, "include", "h2v_hints.h")).read()
    head = text[:text.index("#ifndef H2V_HINTS_H")]
    assert '#include "h2v.h"' in text and "one thread at a time" in head
    assert "depend on the uploaded proofs, instances and draws only" in head and "change its time and nothing else" in head


def test_the_new_bodies_take_no_context_lock():
    """tests/test_thread_scenes_host.py derives the entry points that reach a context's lock from the sources: none of these"""
    import test_thread_scenes_host as scenes
    _, reach, defs = scenes.lock_takers()
    assert set(NAMES) <= set(defs)
    assert not set(NAMES) & reach, sorted(set(NAMES) & reach)


def test_null_batch_is_refused_before_any_device_work(lib):
    vp, sz = ctypes.c_void_p, ctypes.c_size_t
    n = sz(7)
    assert lib.h2v_batch_set_hints(vp(None), sz(1), b"\0" * 32) == -16 and b"h2v_batch_set_hints" in lib.h2v_last_error()
    assert lib.h2v_batch_set_hints_device(vp(None), sz(1), vp(4096), sz(32)) == -16 and b"h2v_batch_set_hints_device" in lib.h2v_last_error()
    assert lib.h2v_batch_hints(vp(None), sz(0), sz(1), ctypes.create_string_buffer(32)) == -16 and b"h2v_batch_hints" in lib.h2v_last_error()
    assert lib.h2v_batch_hints_device(vp(None), sz(0), sz(1), vp(4096), sz(32)) == -16
    assert lib.h2v_batch_hint_stats(vp(None), ctypes.byref(n), ctypes.byref(n), ctypes.byref(n)) == -16 and n.value == 7
    assert lib.h2v_hints_point_offsets(vp(None), None, sz(0), ctypes.byref(n)) == -16


def test_cpp_mirror_header_compiles(tmp_path):
    src = tmp_path / "use_hints.cpp"
    src.write_text('#include "h2v_hints.hpp"\n'
                   "int main() {\n"
                   "    h2v_batch* b = nullptr;\n"
                   "    try {\n"
                   "        std::vector<size_t> off = h2v::hints::point_offsets(nullptr);\n"
                   "        h2v::Bytes y = h2v::hints::for_proofs(off, h2v::Bytes(64), 64);\n"
                   "        std::vector<uint8_t> decoded;\n"
                   "        y = h2v::hints::from_points(h2v::Bytes(32), &decoded);\n"
                   "        h2v::hints::set(b, 1, y);\n"
                   "        h2v::hints::drop(b, 1);\n"
                   "        h2v::hints::set_device(b, 1, nullptr, 32);\n"
                   "        y = h2v::hints::of_launch(b, 0, 1, off.size());\n"
                   "        h2v::hints::of_launch_device(b, 0, 1, nullptr, 32);\n"
                   "        h2v::hints::Stats s = h2v::hints::stats(b);\n"
                   "        return (int)(s.points + s.hinted + s.missed + y.size());\n"
                   "    } catch (const h2v::Failure&) { return 0; }\n"
                   "}\n")
    caller_harness.check_syntax(src)


# ------------------------------------------------------------------ h2v_hints_from_points against the rule in Python integers
def _from_points(lib, points):
    k = len(points)
    y, dec = ctypes.create_string_buffer(max(32 * k, 1)), ctypes.create_string_buffer(max(k, 1))
    assert lib.h2v_hints_from_points(b"".join(points), ctypes.c_size_t(k), y, dec) == 0
    return [y.raw[32 * i:32 * i + 32] for i in range(k)], [dec.raw[i] for i in range(k)]


def _expect(points):
    ys = [hr.decode(pt) for pt in points]
    return [hr.le32(y or 0) for y in ys], [0 if y is None else 1 for y in ys]


def test_from_points_is_the_reference_decode(lib):
    rnd = random.Random(20240)
    valid = [hr.random_point(rnd) for _ in range(200)]
    assert {pt[31] & 0x40 for pt in valid} == {0, 0x40}                    # both sign flags
    nonres = hr.non_residue_x(rnd.randrange(hr.P))
    cases = valid + [hr.encode(nonres, 0), hr.encode(nonres, 1),           # x^3 + 3 a non-residue, found by search
                     hr.encode(hr.P, 0), hr.encode(hr.P + 1, 1),           # x = p, x > p
                     hr.encode((1 << 254) - 1, 0),                         # the largest x under a cleared flag byte
                     hr.encode(0, 0, identity=1), hr.encode(0, 1, identity=1), bytes(valid[0][:31]) + bytes([valid[0][31] | 0x80]),   # the identity flag
                     bytes(32)]                                            # the all-zero string: x = 0
    got_y, got_dec = _from_points(lib, cases)
    want_y, want_dec = _expect(cases)
    assert got_dec == want_dec and got_y == want_y
    assert want_dec[:200] == [1] * 200 and want_dec[200:208] == [0] * 8   # (the cases are what they are named for)
    for pt, y in zip(valid, got_y):
        assert hr.is_hit(pt, y) and (y[0] & 1) == (1 if pt[31] & 0x40 else 0)
    # the Python mirror over the same call
    from halo2_verifier_amd import hints
    y32, decoded = hints.from_points(b"".join(cases))
    assert y32 == b"".join(want_y) and decoded == [bool(v) for v in want_dec]


def test_from_points_edges(lib):
    sz = ctypes.c_size_t
    assert lib.h2v_hints_from_points(None, sz(0), None, None) == 0                       # n = 0: nothing is read
    pt = hr.random_point(random.Random(3))
    y = ctypes.create_string_buffer(32)
    assert lib.h2v_hints_from_points(pt, sz(1), y, None) == 0 and y.raw == hr.le32(hr.decode(pt))   # decoded may be NULL
    assert lib.h2v_hints_from_points(None, sz(1), y, None) == -16 and b"h2v_hints_from_points" in lib.h2v_last_error()
    assert lib.h2v_hints_from_points(pt, sz(1), None, None) == -16
    from halo2_verifier_amd import hints
    assert hints.from_points(b"") == (b"", [])
    with pytest.raises(ValueError, match="32-byte"):
        hints.from_points(b"\0" * 33)


def test_for_proofs_is_the_reference_rows():
    from halo2_verifier_amd import hints
    rnd = random.Random(5)
    offsets, proof_len = [0, 64, 160], 192
    proofs = []
    for i in range(5):
        proof = bytearray(rnd.randrange(256) for _ in range(proof_len))
        for o in offsets:
            proof[o:o + 32] = hr.random_point(rnd)
        proofs.append(bytes(proof))
    bad = bytearray(proofs[3]); bad[64:96] = hr.encode(hr.P, 0); proofs[3] = bytes(bad)
    assert hints.for_proofs(offsets, b"".join(proofs), proof_len) == hr.rows(offsets, proofs)
    with pytest.raises(ValueError, match="whole number"):
        hints.for_proofs(offsets, b"".join(proofs)[:-1], proof_len)
    with pytest.raises(ValueError, match="outside the proof"):
        hints.for_proofs([176], b"".join(proofs), proof_len)


# ------------------------------------------------------------------ Python-side refusals, without a library call
class _Dev:
    def __init__(self, type="cuda", index=0): self.type, self.index = type, index


class _Tensor:
    def __init__(self, shape, stride=None, dtype="torch.uint8", device=None):
        self.shape, self._stride, self.dtype, self.device = shape, stride or (shape[-1], 1), dtype, device or _Dev()
    def stride(self): return self._stride
    def data_ptr(self): return 0x7f0000000000


def _bare_batch(monkeypatch, n=10, n_points=3):
    from halo2_verifier_amd import hints, verifier

    def no_library():
        raise AssertionError("the library was reached")
    monkeypatch.setattr(hints, "_library", no_library)
    b = verifier.Batch.__new__(verifier.Batch)
    b.n, b._keep, b._hint_points = n, None, n_points
    b.ctx = types.SimpleNamespace(device=0)
    return b


def test_python_refuses_wrong_lengths_and_tensors_without_the_library(monkeypatch):
    b = _bare_batch(monkeypatch)                     # rows of 96 bytes, 10 proofs
    for size in (0, 959, 961, 96):
        with pytest.raises(ValueError, match="960 bytes"):
            b.set_hints(b"\0" * size)
    with pytest.raises(TypeError, match="uint8"):
        b.set_hints_tensor(_Tensor((10, 96), dtype="torch.int32"))
    with pytest.raises(ValueError, match="context's device"):
        b.set_hints_tensor(_Tensor((10, 96), device=_Dev(index=1)))
    with pytest.raises(ValueError, match="10 rows"):
        b.set_hints_tensor(_Tensor((9, 96)))
    with pytest.raises(ValueError, match="rows of 32 \\* n_points = 96"):
        b.set_hints_tensor(_Tensor((10, 128)))
    with pytest.raises(ValueError, match="multiple of 16"):
        b.set_hints_tensor(_Tensor((10, 96), stride=(104, 1)))
    with pytest.raises(ValueError, match="overlap"):
        b.set_hints_tensor(_Tensor((10, 96), stride=(80, 1)))      # a stride below 32 Np
    with pytest.raises(ValueError, match="2-D"):
        b.set_hints_tensor(_Tensor((960,), stride=(1,)))
    with pytest.raises(TypeError, match="tensor"):
        b.set_hints_tensor(b"\0" * 960)
    with pytest.raises(ValueError, match="multiple of 16"):
        b.hints_into(_Tensor((4, 96), stride=(100, 1)), 2, 4)
    with pytest.raises(ValueError, match="4 rows"):
        b.hints_into(_Tensor((5, 96)), 2, 4)
    with pytest.raises(TypeError, match="uint8"):
        b.hints_into(_Tensor((4, 96), dtype="torch.int8"), 2, 4)


def test_python_refuses_ranges_outside_the_upload_without_the_library(monkeypatch):
    b = _bare_batch(monkeypatch)
    for call in (lambda f, c: b.hints(f, c), lambda f, c: b.hints_into(_Tensor((max(c, 1) if isinstance(c, int) else 1, 96)), f, c)):
        for first, count in ((11, 0), (0, 11), (4, 7), (10, 1), (-1, 2), (0, -1), (2**64, 0)):
            with pytest.raises(ValueError):
                call(first, count)
        for first, count in ((1.5, 1), (0, "2"), (True, 1)):
            with pytest.raises(TypeError):
                call(first, count)
    assert b.hints(10, None) == b"" and b.hints(3, 0) == b""        # an empty range: nothing to ask the library
