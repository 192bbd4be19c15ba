"""Draws from a seed, on the host: h2v_draws_expand (the library's own BLAKE2b single-block compression and the Fr reduction)
against the definition in hashlib, its refusals, and where the two entry points are declared and exported.  The device kernel is
tests/test_gpu_draws.py's."""
import ctypes
import hashlib
import os
import re
import subprocess

import pytest

import caller_harness

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
SEED_A = bytes(range(32))
SEED_B = bytes((7 * i + 3) % 256 for i in range(32))


def ref_draw(seed, i):
    """the issue's expression, as it stands"""
    return int.from_bytes(hashlib.blake2b(seed + i.to_bytes(8, 'little'), digest_size=64, person=b'h2v-draws-v1').digest(), 'little') % R_MOD


def ref_expand(seed, first, n):
    return b"".join(ref_draw(seed, first + j).to_bytes(32, "little") for j in range(n))


@pytest.fixture(scope="module")
def lib():
    import halo2_verifier_amd as h2v
    if not os.path.exists(h2v.lib_path()):
        subprocess.check_call(["make", "-j", "4", "-C", os.path.join(ROOT, "halo2_verifier_amd", "csrc")])
    lib = ctypes.CDLL(h2v.lib_path())
    lib.h2v_draws_expand.restype = ctypes.c_int
    lib.h2v_draws_expand.argtypes = [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_char_p]
    lib.h2v_last_error.restype = ctypes.c_char_p
    return lib


def c_expand(lib, seed, first, n):
    out = ctypes.create_string_buffer(b"\xa5" * (32 * n + 32), 32 * n + 32)
    rc = lib.h2v_draws_expand(seed, first, n, out)
    assert out.raw[32 * n:] == b"\xa5" * 32      # nothing written past the n draws
    return rc, out.raw[:32 * n]


ANCHORS = [
    (SEED_A, 0, 0x0607e6c5ce8f7375ea1844befb5daf4254965d7eb09a39d6c4517fcdd083a836),
    (SEED_A, 2**32, 0x0868191628889fa2ded1674ca5f3c1224c59425f1d4237d514fcb7f05d9bd118),
    (bytes(32), 2**64 - 1, 0x18dac5e3375e9e19c02fd8bc5fec5b0dd086a06209773b32d1f170ea7301574e),
]


@pytest.mark.parametrize("seed,i,value", ANCHORS)
def test_anchors(lib, seed, i, value):
    assert ref_draw(seed, i) == value                       # the definition itself
    rc, got = c_expand(lib, seed, i, 1)
    assert rc == 0 and int.from_bytes(got, "little") == value


@pytest.mark.parametrize("first,n", [(0, 0), (0, 1), (0, 17), (5, 1000), (2**32 - 3, 8), (2**64 - 4, 4)])
def test_expand_matches_hashlib(lib, first, n):
    for seed in (SEED_A, SEED_B):
        rc, got = c_expand(lib, seed, first, n)
        assert rc == 0 and got == ref_expand(seed, first, n)
    # every draw is canonical
    assert all(int.from_bytes(got[32 * j:32 * j + 32], "little") < R_MOD for j in range(n))


def test_python_expand_is_the_library_and_slices_agree():
    import halo2_verifier_amd as h2v
    from halo2_verifier_amd import draws
    assert h2v.expand is draws.expand and h2v.expand_tensor is draws.expand_tensor and h2v.new_seed is draws.new_seed
    for a, m, k in [(0, 0, 5), (0, 16, 1), (3, 17, 40), (2**32 - 2, 1, 4), (2**64 - 9, 4, 5)]:
        whole = draws.expand(SEED_B, a, m + k)
        assert whole == draws.expand(SEED_B, a, m) + draws.expand(SEED_B, a + m, k) == ref_expand(SEED_B, a, m + k)
    assert draws.draw(SEED_A, 0) == ANCHORS[0][2].to_bytes(32, "little")
    s1, s2 = draws.new_seed(), draws.new_seed()
    assert len(s1) == len(s2) == 32 and s1 != s2


def test_refusals(lib):
    out = ctypes.create_string_buffer(32 * 8)
    for first, n in [(2**64 - 4, 5), (2**64 - 1, 2), (2, 2**64 - 1)]:
        assert lib.h2v_draws_expand(SEED_A, first, n, out) == -16
        assert b"wraps" in lib.h2v_last_error()
    assert lib.h2v_draws_expand(None, 0, 1, out) == -16 and b"null" in lib.h2v_last_error()
    assert lib.h2v_draws_expand(SEED_A, 0, 1, None) == -16 and b"null" in lib.h2v_last_error()
    assert lib.h2v_draws_expand(SEED_A, 0, 0, None) == 0          # nothing to write
    assert lib.h2v_draws_expand(SEED_A, 2**64 - 4, 4, out) == 0   # up to the last index
    # the device form refuses a range longer than one launch holds before it looks at the device or the pointer (so also without a GPU)
    text = open(os.path.join(ROOT, "include", "h2v_draws.h")).read()
    limit = int(re.search(r"#define H2V_DRAWS_DEVICE_MAX (\d+)", text).group(1))
    assert limit == (2**26 - 1) * 16 and (limit // 16) * 64 < 2**32 <= (limit // 16 + 1) * 64
    lib.h2v_draws_expand_device.restype = ctypes.c_int
    lib.h2v_draws_expand_device.argtypes = [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p]
    assert lib.h2v_draws_expand_device(0, None, SEED_A, 0, limit + 1, ctypes.c_void_p(4096)) == -16
    assert b"H2V_DRAWS_DEVICE_MAX" in lib.h2v_last_error()
    from halo2_verifier_amd import draws
    with pytest.raises(ValueError):
        draws.expand(SEED_A, 2**64 - 4, 5)
    with pytest.raises(ValueError):
        draws.expand(SEED_A[:31], 0, 1)
    with pytest.raises(TypeError):
        draws.expand("0" * 32, 0, 1)
    with pytest.raises(ValueError):
        draws.expand(SEED_A, -1, 1)
    rs = open(os.path.join(ROOT, "integration", "rust", "draws.rs")).read()
    assert draws.DEVICE_MAX == limit == int(re.search(r"pub const H2V_DRAWS_DEVICE_MAX: usize = (\d+);", rs).group(1))


def test_python_falls_back_to_hashlib_only_when_the_library_cannot_load(monkeypatch):
    from halo2_verifier_amd import _lib, draws

    def missing():
        raise OSError("cannot open shared object file")
    monkeypatch.setattr(draws, "_BOUND", None)
    monkeypatch.setattr(_lib, "load_library", missing)
    assert draws.expand(SEED_A, 2**32 - 3, 8) == ref_expand(SEED_A, 2**32 - 3, 8)

    class Failing:
        def h2v_draws_expand(self, *a):
            return -18

        def h2v_last_error(self):
            return b"h2v_draws_expand: failed"
    monkeypatch.setattr(draws, "_BOUND", Failing())
    monkeypatch.setattr(_lib, "load_library", lambda: Failing())
    with pytest.raises(_lib.H2VError):       # a failing library is an error, never replaced by other draws
        draws.expand(SEED_A, 0, 1)


def _declared(header):
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", header)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(h2v_[a-z0-9_]+)\s*\(", text)))


def test_symbols_are_exported_declared_in_their_own_header_and_bound(lib):
    from halo2_verifier_amd import _lib, draws
    names = ["h2v_draws_expand", "h2v_draws_expand_device"]
    assert _declared("h2v_draws.h") == names
    assert all(hasattr(lib, n) for n in names)
    assert not set(names) & set(_declared("h2v.h")) and not set(names) & set(_lib.SIGNATURES)
    assert sorted(draws.SIGNATURES) == names
    rs = open(os.path.join(ROOT, "integration", "rust", "draws.rs")).read()
    assert sorted(set(re.findall(r"pub fn (h2v_[a-z0-9_]+)\s*\(", rs))) == names
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.lib_path()], capture_output=True, text=True, check=True).stdout
    assert all(re.search(r" T %s$" % n, out, re.M) for n in names)


def test_batch_and_shard_keywords_refuse_both_forms():
    """rand_tail and seed together is a ValueError, before anything is looked at"""
    from halo2_verifier_amd import verifier, distributed
    b = verifier.Batch.__new__(verifier.Batch)
    with pytest.raises(ValueError, match="not both"):
        b.upload_tensors(None, None, [], rand_tail=object(), seed=SEED_A)
    with pytest.raises(ValueError, match="not both"):
        b.upload(b"", 0, b"", [], rand_tail=b"", seed=SEED_A)
    with pytest.raises(ValueError, match="go with seed"):
        b.upload_tensors(None, None, [], first_index=3)
    sb = distributed.ShardedBatch.__new__(distributed.ShardedBatch)
    with pytest.raises(ValueError, match="not both"):
        sb.upload_tensors(None, None, [], rand_tail=object(), seed=SEED_A, lo=0, total=1)
    with pytest.raises(ValueError, match="lo and total"):
        sb.upload_tensors(None, None, [], seed=SEED_A)
    assert distributed.seeded_tail(SEED_A, 3, 10, 2) == ref_expand(SEED_A, 3, 7) + ref_expand(SEED_A, 13, 7)


def test_cpp_mirror_header_compiles(tmp_path):
    src = tmp_path / "use_draws.cpp"
    src.write_text('#include "h2v_draws.hpp"\n'
                   "int main() {\n"
                   "    std::array<uint8_t, 32> seed{};\n"
                   "    std::vector<uint8_t> d = h2v::draws::expand(seed, 5, 3);\n"
                   "    h2v::draws::expand_device(0, nullptr, seed, 0, 0, nullptr);\n"
                   "    return d.size() == 96 ? 0 : 1;\n"
                   "}\n")
    caller_harness.check_syntax(src)
