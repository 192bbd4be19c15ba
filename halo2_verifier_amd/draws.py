"""Draws from a seed: ctypes binding of include/h2v_draws.h, and the tensors a device-resident or sharded batch takes from it.

The per-proof Fr::random draws of a batch are the expansion of one 32-byte secret seed:

    draw(seed, i) = LE512(BLAKE2b-512(seed | LE64(i), digest 64, no key, personal b"h2v-draws-v1")) mod r      (32 canonical bytes)

so a batch whose proofs live in device memory, or one sharded over GPUs, needs 32 bytes instead of 32 per proof.  The seed comes
from the OS RNG (new_seed), is chosen independently of the proofs and is not revealed to provers before the verdict.

  expand(seed, first, n)                      the draws of indices [first, first + n) as bytes, on the host
  expand_tensor(seed, first, n, device, ...)  the same as a uint8 tensor [n, 32] in device memory, by one kernel on a stream
  new_seed()                                  32 bytes from the OS

The two C entry points are context-free (no context, no lock, no shared state): any number of threads may call them at once.
"""
import ctypes
import hashlib
import numbers
import os

from . import _lib

R_MODULUS = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
PERSONAL = b"h2v-draws-v1"
DEVICE_MAX = 1073741808   # include/h2v_draws.h H2V_DRAWS_DEVICE_MAX: the most draws one device call expands

# the symbols include/h2v_draws.h declares: (restype, argtypes).  A table of its own beside _lib.SIGNATURES, which mirrors include/h2v.h
SIGNATURES = {
    "h2v_draws_expand": (ctypes.c_int, [ctypes.c_char_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_char_p]),
    "h2v_draws_expand_device": (ctypes.c_int, [ctypes.c_int, ctypes.c_void_p, ctypes.c_char_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p]),
}
_BOUND = None


def _library():
    """The loaded library with this module's symbols bound (AttributeError: a library built before they existed)."""
    global _BOUND
    if _BOUND is None:
        lib = _lib.load_library()
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _BOUND = lib
    return _BOUND


def new_seed() -> bytes:
    """A fresh seed: 32 bytes from the OS RNG."""
    return os.urandom(32)


def _seed_bytes(seed) -> bytes:
    if not isinstance(seed, (bytes, bytearray, memoryview)):
        raise TypeError(f"a seed is 32 bytes, got {type(seed).__name__}")
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError(f"a seed is 32 bytes, got {len(seed)}")
    return seed


def _range(first, n):
    for v, what in ((first, "first"), (n, "n")):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise TypeError(f"{what} must be an integer, got {type(v).__name__}")
    first, n = int(first), int(n)
    if first < 0 or n < 0 or first >> 64:
        raise ValueError(f"first must be in [0, 2^64) and n >= 0, got {first} and {n}")
    if first + n > 1 << 64:
        raise ValueError(f"first + n = {first + n} is beyond 2^64: a draw's index is 64 bits")
    return first, n


def draw(seed: bytes, i: int) -> bytes:
    """The definition, in hashlib: draw i of `seed` as 32 canonical little-endian bytes."""
    digest = hashlib.blake2b(seed + i.to_bytes(8, "little"), digest_size=64, person=PERSONAL).digest()
    return (int.from_bytes(digest, "little") % R_MODULUS).to_bytes(32, "little")


def expand(seed, first: int, n: int) -> bytes:
    """draw(seed, first) | .. | draw(seed, first + n - 1): n * 32 bytes, computed on the host (h2v_draws_expand)."""
    seed = _seed_bytes(seed)
    first, n = _range(first, n)
    try:
        lib = _library()
    except (_lib.H2VError, OSError, AttributeError):   # library missing or stale (orchestration tests without the product): the definition itself
        return b"".join(draw(seed, first + j) for j in range(n))
    buf = ctypes.create_string_buffer(max(32 * n, 1))
    _lib.check(lib.h2v_draws_expand(seed, first, n, buf))
    return buf.raw[: 32 * n]


def _stream_handle(stream, device):
    """(raw HIP stream handle, whether it is torch's current stream of `device`) of a torch.cuda.Stream, a raw handle or None = current"""
    import torch
    current = torch.cuda.current_stream(device).cuda_stream
    if stream is None:
        return current, True
    handle = stream.cuda_stream if hasattr(stream, "cuda_stream") else int(stream)
    return handle, handle == current


def expand_into(seed, first: int, out, stream=None):
    """The draws of indices [first, first + len(out)) into `out`, a contiguous uint8 tensor [n, 32] in device memory, by one kernel
    (k_expand_draws) on `stream`: a torch.cuda.Stream, a raw HIP stream handle, or None = torch's current stream of out's device.
    Waits for nothing on the host.  On a stream other than the current one, that stream is first made to wait (on the device) for
    the work queued on the current one — `out` may be memory that work still uses.  Given a torch.cuda.Stream, `out` is also marked
    as used on it (record_stream), so its memory is not handed out again before the kernel has run.  Given a raw handle it is not:
    the allocator would record an event on that stream when `out` is freed, and a raw stream may be gone by then (a batch's own
    stream goes with the batch) — the caller keeps `out` referenced until the work on that stream has run, as a batch does for a
    seed's tail (Batch.hold_tail: an event on its stream behind the upload)."""
    import torch
    seed = _seed_bytes(seed)
    if out.dtype != torch.uint8 or out.device.type != "cuda" or out.dim() != 2 or out.shape[1] != 32 or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor [n, 32] in device memory, got {out.dtype} {tuple(out.shape)} on {out.device}")
    first, n = _range(first, out.shape[0])
    if n > DEVICE_MAX:
        raise ValueError(f"one call expands at most {DEVICE_MAX} draws into device memory, got {n}: expand the range in pieces")
    lib = _library()
    handle, is_current = _stream_handle(stream, out.device)
    if not is_current:
        external = torch.cuda.ExternalStream(handle, device=out.device)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(out.device))
        external.wait_event(ev)
        if hasattr(stream, "cuda_stream"):
            out.record_stream(stream)
    _lib.check(lib.h2v_draws_expand_device(out.device.index, ctypes.c_void_p(handle), seed, first, n, ctypes.c_void_p(out.data_ptr() if n else 0)))
    return out


def expand_tensor(seed, first: int, n: int, device, stream=None):
    """expand() into device memory -> uint8 tensor [n, 32] on `device` (an index, a string or a torch.device), written by one kernel
    on `stream` (expand_into's rules; None = torch's current stream).  No host wait, and no bytes cross to the device but the seed,
    which travels in the kernel's arguments."""
    import torch
    _seed_bytes(seed)
    first, n = _range(first, n)
    if n > DEVICE_MAX:
        raise ValueError(f"one call expands at most {DEVICE_MAX} draws into device memory, got {n}: expand the range in pieces")
    device = torch.device("cuda", device) if isinstance(device, numbers.Integral) else torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"expand_tensor writes device memory, got {device}")
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    out = torch.empty((n, 32), dtype=torch.uint8, device=device)
    return expand_into(seed, first, out, stream)
