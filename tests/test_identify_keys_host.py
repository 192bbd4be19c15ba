"""h2v_verify_batch_keys_identify and h2v_batches_recheck without a GPU: both symbols are declared, exported and bound, and the
argument checks that come before any device work refuse null arrays and an empty key or batch set, writing nothing."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = -16
NAMES = ("h2v_verify_batch_keys_identify", "h2v_batches_recheck")


def test_header_declares_and_library_exports_the_new_entry_points():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "h2v.h")).read(), flags=re.S)
    from halo2_verifier_amd import _lib
    so = ctypes.CDLL(_lib.lib_path())
    rs = open(os.path.join(ROOT, "integration", "rust", "ffi.rs")).read()
    for name in NAMES:
        assert re.search(r"\bint %s\s*\(" % name, text), name
        assert hasattr(so, name), name
        assert name in _lib.SIGNATURES, name
        assert re.search(r"pub fn %s\s*\(" % name, rs), name


def _identify(lib, ctxs, n_keys, keys, n):
    """h2v_verify_batch_keys_identify with no proofs behind the pointers -> (rc, outputs after the call)"""
    PA = ctypes.c_char_p * max(n, 1)
    proofs = PA(*([b"\0" * 8] * n)) if n else PA()
    lens = (ctypes.c_size_t * max(n, 1))(*([8] * n))
    ncols = (ctypes.c_size_t * 1)(1)
    cl = (ctypes.c_size_t * max(n, 1))(*([1] * n))
    st = (ctypes.c_int * max(n, 1))(*([5] * max(n, 1)))
    ok, checks = ctypes.c_int(7), ctypes.c_size_t(9)
    left, right = ctypes.create_string_buffer(b"\x11" * 64, 64), ctypes.create_string_buffer(b"\x22" * 64, 64)
    rc = lib.h2v_verify_batch_keys_identify(ctxs, n_keys, keys, n, proofs, lens, PA(), ncols, cl, None, st, ctypes.byref(ok), left, right,
                                            ctypes.byref(checks))
    return rc, (list(st), ok.value, checks.value, left.raw, right.raw)


UNTOUCHED = ([5, 5], 7, 9, b"\x11" * 64, b"\x22" * 64)


def test_keys_identify_refuses_null_contexts_null_keys_and_no_keys():
    from halo2_verifier_amd import _lib
    lib = _lib.load_library()
    keys = (ctypes.c_uint32 * 2)(0, 0)
    # a null context array
    rc, out = _identify(lib, None, 1, keys, 2)
    assert rc == BAD_ARGUMENT and out == UNTOUCHED
    assert "h2v_verify_batch_keys_identify" in _lib.last_error()
    # no keys
    ctxs = (ctypes.c_void_p * 1)(None)
    rc, out = _identify(lib, ctxs, 0, keys, 2)
    assert rc == BAD_ARGUMENT and out == UNTOUCHED
    # a null key index array with proofs
    rc, out = _identify(lib, ctxs, 1, None, 2)
    assert rc == BAD_ARGUMENT and out == UNTOUCHED
    assert "h2v_verify_batch_keys_identify" in _lib.last_error()
    # a null context inside the array
    rc, out = _identify(lib, ctxs, 1, keys, 2)
    assert rc == BAD_ARGUMENT and out == UNTOUCHED


def _recheck(lib, batches, n_batches, bor, n_ranges):
    first = (ctypes.c_size_t * 2)(0, 1)
    count = (ctypes.c_size_t * 2)(1, 1)
    ok = (ctypes.c_int * 2)(7, 7)
    left, right = ctypes.create_string_buffer(b"\x11" * 128, 128), ctypes.create_string_buffer(b"\x22" * 128, 128)
    rc = lib.h2v_batches_recheck(batches, n_batches, n_ranges, bor, first, count, ok, left, right)
    return rc, (list(ok), left.raw, right.raw)


def test_batches_recheck_refuses_null_batches_null_indices_and_no_batches():
    from halo2_verifier_amd import _lib
    lib = _lib.load_library()
    untouched = ([7, 7], b"\x11" * 128, b"\x22" * 128)
    bor = (ctypes.c_uint32 * 2)(0, 0)
    rc, out = _recheck(lib, None, 1, bor, 2)
    assert rc == BAD_ARGUMENT and out == untouched
    assert "h2v_batches_recheck" in _lib.last_error()
    batches = (ctypes.c_void_p * 2)(None, None)
    rc, out = _recheck(lib, batches, 0, bor, 2)
    assert rc == BAD_ARGUMENT and out == untouched
    # a null index array, checked before the batches are looked at
    rc, out = _recheck(lib, batches, 2, None, 2)
    assert rc == BAD_ARGUMENT and out == untouched
    assert "null argument" in _lib.last_error()
    # a null batch in the array (no batch is Finished)
    rc, out = _recheck(lib, batches, 2, bor, 2)
    assert rc == BAD_ARGUMENT and out == untouched
    assert "h2v_batches_recheck" in _lib.last_error()
    # with no ranges the null batch is still refused
    rc, out = _recheck(lib, batches, 1, None, 0)
    assert rc == BAD_ARGUMENT and out == untouched


def test_python_api_refuses_empty_lists_before_calling_in():
    import halo2_verifier_amd as h2v
    for call in (lambda: h2v.verify_batch_keys_identify([], [], [], []), lambda: h2v.recheck_batches([], [(0, 0, 1)])):
        try:
            call()
        except ValueError:
            pass
        else:
            raise AssertionError("an empty list was not refused")
