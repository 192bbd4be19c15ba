"""h2v_verify_batch_keys without a GPU: the symbol is declared and exported, and the argument checks that come before any device
work refuse a null context array and an empty key set."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARGUMENT = -16


def test_header_declares_and_library_exports_verify_batch_keys():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "h2v.h")).read(), flags=re.S)
    assert re.search(r"\bint h2v_verify_batch_keys\s*\(", text)
    from halo2_verifier_amd import _lib
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "h2v_verify_batch_keys")
    assert "h2v_verify_batch_keys" in _lib.SIGNATURES


def test_null_contexts_and_no_keys_are_refused_without_a_device():
    from halo2_verifier_amd import _lib
    import halo2_verifier_amd as h2v
    lib = _lib.load_library()
    st, ok = (ctypes.c_int * 1)(), ctypes.c_int(7)
    ncols = (ctypes.c_size_t * 1)(1)
    assert lib.h2v_verify_batch_keys(None, 1, None, 0, None, None, None, ncols, None, None, st, ctypes.byref(ok), None, None) == BAD_ARGUMENT
    ctxs = (ctypes.c_void_p * 1)(None)
    assert lib.h2v_verify_batch_keys(ctxs, 0, None, 0, None, None, None, ncols, None, None, st, ctypes.byref(ok), None, None) == BAD_ARGUMENT
    assert "h2v_verify_batch_keys" in _lib.last_error()
    assert ok.value == 7   # nothing was written
    # the Python API refuses an empty context list before calling in
    try:
        h2v.verify_batch_keys([], [], [], [])
    except ValueError:
        pass
    else:
        raise AssertionError("verify_batch_keys([]) did not raise")
