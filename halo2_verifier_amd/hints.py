"""Point hints: ctypes binding of include/h2v_hints.h (a staged batch: Batch.set_hints, .set_hints_tensor, .hints, .hints_into,
.hint_stats) and of include/h2v_hint_rows.h (a row per proof or None: Batch.set_hint_rows, and the hints= keyword of
Context.verify_batch, Context.verify_batches, verify_batch_keys, Accumulator.process and verify_proof with an AccumulatorStrategy).

Every launch of a Batch decodes every compressed G1 point of every proof, a square root in Fq per point.  Whoever sends a proof knows
both coordinates of its points.  A hint is the claimed y of a point, 32 canonical little-endian bytes; a hint row holds the y of the
Np points of one proof in byte order (point_offsets).  The encoding fixes y completely, so a hint is checked, never trusted: where it
holds, the point costs a curve check; where it does not, the square root it would have paid anyway.

The invariant: the results of a launch depend on the uploaded proofs, instances and draws only.  The hints, whatever bytes they
hold, change its time and nothing else.

  point_offsets(ctx)                         the byte offsets of the Np points inside a proof of the context's key
  from_points(points)                        the y of compressed points, on the host (no device) -> (y32 bytes, decoded flags)
  for_proofs(offsets, proofs_flat, proof_len)  the hint rows of whole proofs -> n * Np * 32 bytes
  set_hints / set_hints_device / set_hints_tensor   the hints of the batch's current upload, from host or device memory
  hints / hints_device / hints_into          the canonical y a launch leaves behind: hints for the next verifier of the same proofs
  hint_stats                                 (n_points, n_hinted, n_missed) of the last launch
  set_hint_rows                              the same from one row per proof, None where a sender gave none
  call_rows(contexts, keys, hints)           the checked row array of a one-shot call's hints= keyword (verifier.py)

Cost: 32 bytes per point beside the proof.  A sender of bad hints gets the speed of a launch without hints plus the check; the
points without a usable hint, whichever proofs they belong to, have their roots taken together behind the check.
"""
import ctypes

from . import _lib

c_vp, c_sz, c_int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
c_szp = ctypes.POINTER(c_sz)

# the symbols include/h2v_hints.h declares: (restype, argtypes).  A table of its own beside _lib.SIGNATURES, which mirrors include/h2v.h
SIGNATURES = {
    "h2v_hints_point_offsets": (c_int, [c_vp, c_szp, c_sz, c_szp]),
    "h2v_hints_from_points": (c_int, [ctypes.c_char_p, c_sz, ctypes.c_char_p, ctypes.c_char_p]),
    "h2v_batch_set_hints": (c_int, [c_vp, c_sz, ctypes.c_char_p]),
    "h2v_batch_set_hints_device": (c_int, [c_vp, c_sz, c_vp, c_sz]),
    "h2v_batch_hints": (c_int, [c_vp, c_sz, c_sz, ctypes.c_char_p]),
    "h2v_batch_hints_device": (c_int, [c_vp, c_sz, c_sz, c_vp, c_sz]),
    "h2v_batch_hint_stats": (c_int, [c_vp, c_szp, c_szp, c_szp]),
}
# and include/h2v_hint_rows.h: a row per proof or none.  hint_rows after proof_lens, hint_stats (size_t[3]) last
_u8pp, _u32p, _vpp, _intp = ctypes.POINTER(ctypes.c_char_p), ctypes.POINTER(ctypes.c_uint32), ctypes.POINTER(c_vp), ctypes.POINTER(c_int)
ROW_SIGNATURES = {
    "h2v_batch_set_hint_rows": (c_int, [c_vp, c_sz, _u8pp]),
    "h2v_verify_batch_keys_hinted": (c_int, [_vpp, c_sz, _u32p, c_sz, _u8pp, c_szp, _u8pp, _u8pp, c_szp, c_szp, ctypes.c_char_p, _intp, _intp, ctypes.c_char_p,
                                             ctypes.c_char_p, c_szp]),
    "h2v_verify_batches_hinted": (c_int, [c_vp, c_sz, c_szp, _u8pp, c_szp, _u8pp, _u8pp, c_sz, c_szp, ctypes.c_char_p, _intp, _intp, ctypes.c_char_p, ctypes.c_char_p,
                                          c_szp]),
    "h2v_accumulator_process_hinted": (c_int, [c_vp, _vpp, c_sz, _u32p, c_sz, _u8pp, c_szp, _u8pp, _u8pp, c_szp, c_szp, ctypes.c_char_p, _intp, _intp, c_szp]),
}
_BOUND = None


def _library():
    """The loaded library with this module's symbols bound (AttributeError: a library built before they existed)."""
    global _BOUND
    if _BOUND is None:
        lib = _lib.load_library()
        for name, (res, args) in list(SIGNATURES.items()) + list(ROW_SIGNATURES.items()):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
        _BOUND = lib
    return _BOUND


# ---- host only: what a sender without a GPU uses
def point_offsets(ctx):
    """-> the byte offsets of the Np compressed points inside a proof of the context's key, ascending (h2v_hints_point_offsets)"""
    n = c_sz(0)
    _lib.check(_library().h2v_hints_point_offsets(ctx._h, None, 0, ctypes.byref(n)))
    out = (c_sz * max(n.value, 1))()
    _lib.check(_library().h2v_hints_point_offsets(ctx._h, out, n.value, ctypes.byref(n)))
    return list(out)[:n.value]


def from_points(points):
    """points: k * 32 bytes of compressed G1 points -> (y32, decoded): k * 32 bytes, the canonical y of each point or 32 zero bytes
    where G1Affine::from_bytes fails, and a list of k bools (h2v_hints_from_points; no device, no context)"""
    points = bytes(points)
    if len(points) % 32:
        raise ValueError(f"points must be a whole number of 32-byte points, got {len(points)} bytes")
    k = len(points) // 32
    y, dec = ctypes.create_string_buffer(max(32 * k, 1)), ctypes.create_string_buffer(max(k, 1))
    _lib.check(_library().h2v_hints_from_points(points, k, y, dec))
    return y.raw[:32 * k], [bool(v) for v in dec.raw[:k]]


def for_proofs(offsets, proofs_flat, proof_len):
    """The hint rows of n proofs of proof_len bytes each, their points at `offsets` (point_offsets) -> n * len(offsets) * 32 bytes;
    a point that does not decode gets 32 zero bytes, which is a miss like any other"""
    proofs_flat, offsets = bytes(proofs_flat), [int(o) for o in offsets]
    if proof_len <= 0 or len(proofs_flat) % proof_len:
        raise ValueError("proofs_flat is not a whole number of proofs")
    if any(o < 0 or o + 32 > proof_len for o in offsets):
        raise ValueError("a point offset lies outside the proof")
    n = len(proofs_flat) // proof_len
    points = b"".join(proofs_flat[i * proof_len + o:i * proof_len + o + 32] for i in range(n) for o in offsets)
    return from_points(points)[0]


# ---- on a batch
def _n_points(batch):
    """Np of the batch's context (kept on the batch: it is a fact of the key)"""
    np_ = getattr(batch, "_hint_points", None)
    if np_ is None:
        np_ = batch._hint_points = int(batch.ctx.proof_shape()["n_points"])
    return np_


def _range(batch, first, count):
    from .guards import _range as guards_range
    return guards_range(batch, first, count)


def _stride(row_stride, row_len):
    from .verifier import _integer
    row_stride = _integer(row_stride, "row_stride")
    if row_stride % 16 or row_stride < row_len:
        raise ValueError(f"row_stride must be a multiple of 16 and at least 32 * n_points = {row_len}, got {row_stride}")
    return row_stride


def set_hints(batch, y32):
    """The hints of the batch's current upload from host bytes, n * Np * 32 of them (h2v_batch_set_hints); None drops them.  The
    batch must be uploaded and not launched since."""
    n = int(batch.n)
    if y32 is None:
        _lib.check(_library().h2v_batch_set_hints(batch._h, n, None))
        return
    y32 = bytes(y32)
    want = n * _n_points(batch) * 32
    if len(y32) != want:
        raise ValueError(f"the hints of {n} proofs are n * n_points * 32 = {want} bytes, got {len(y32)}")
    _lib.check(_library().h2v_batch_set_hints(batch._h, n, y32))


def _rows_array(rows, row_lens):
    """rows: a sequence of bytes | None, one per proof; row_lens: the length each must have -> the char* array h2v_hint_rows.h takes.
    Every refusal comes before any library call."""
    if rows is None or isinstance(rows, (bytes, bytearray, str)) or not hasattr(rows, "__len__"):
        raise TypeError("hints must be a sequence of bytes or None, one per proof")
    rows, n = list(rows), len(row_lens)
    if len(rows) != n:
        raise ValueError(f"{n} proofs need {n} hint rows (None for a proof without hints), got {len(rows)}")
    for i, (row, want) in enumerate(zip(rows, row_lens)):
        if row is None:
            continue
        if not isinstance(row, (bytes, bytearray)):
            raise TypeError(f"hint row {i} must be bytes or None, got {type(row).__name__}")
        if len(row) != want:
            raise ValueError(f"hint row {i} must hold n_points * 32 = {want} bytes, got {len(row)}")
    return (ctypes.c_char_p * max(n, 1))(*[None if r is None else bytes(r) for r in rows])


def _points_of(ctx):
    """Np of a context's key (kept on the context: it is a fact of the key)"""
    np_ = getattr(ctx, "_hint_points", None)
    if np_ is None:
        np_ = ctx._hint_points = int(ctx.proof_shape()["n_points"])
    return np_


def call_rows(contexts, keys, rows):
    """The hints= keyword of a one-shot call: rows[i] is proof i's row of 32 Np bytes, Np of contexts[keys[i]], or None -> the array
    the _hinted entry points take (the sequence is sized before a context is asked for its Np)"""
    if rows is not None and hasattr(rows, "__len__") and not isinstance(rows, (bytes, bytearray, str)) and len(rows) != len(keys):
        raise ValueError(f"{len(keys)} proofs need {len(keys)} hint rows (None for a proof without hints), got {len(rows)}")
    return _rows_array(rows, [32 * _points_of(contexts[k]) for k in keys])


def stats_out():
    return (c_sz * 3)()


def expected_stats(n_points_per_proof, rows, missed):
    """What the entry points report for rows given per proof: (points, hinted points, hinted points missed).  n_points_per_proof: Np of
    every proof; rows: per proof a row or None; missed: per proof the hints of its row that the device does not use (0 where rows[i] is
    None) -> the three counters.  The arithmetic of h2v_batch_hint_stats after h2v_batch_set_hint_rows, for tests and probes."""
    points = sum(n_points_per_proof)
    hinted = sum(np_ for np_, r in zip(n_points_per_proof, rows) if r is not None)
    return points, hinted, sum(m for m, r in zip(missed, rows) if r is not None)


def set_hint_rows(batch, rows):
    """The hints of the batch's current upload from one row per proof, None where the proof's sender gave none
    (h2v_batch_set_hint_rows); rows=None drops them.  The batch must be uploaded and not launched since."""
    n = int(batch.n)
    if rows is None:
        _lib.check(_library().h2v_batch_set_hint_rows(batch._h, n, None))
        return
    arr = _rows_array(rows, [32 * _n_points(batch)] * n)
    _lib.check(_library().h2v_batch_set_hint_rows(batch._h, n, arr))


def set_hints_device(batch, addr, row_stride):
    """set_hints from device memory, as an address: row i at addr + i * row_stride, device -> device on the batch's stream, no host
    wait (h2v_batch_set_hints_device).  The caller orders the producer of the rows before the call."""
    from .verifier import _address
    row_stride = _stride(row_stride, _n_points(batch) * 32)
    addr = _address(addr, "the hints' address", needed=batch.n > 0)
    _lib.check(_library().h2v_batch_set_hints_device(batch._h, int(batch.n), c_vp(addr), row_stride))


def _rows_tensor(batch, t, rows, what):
    """a tensor of hint rows: uint8, on the batch's device, [rows, 32 Np] with any row stride that is a multiple of 16"""
    from .verifier import Batch
    row_len = _n_points(batch) * 32
    addr, _, stride = Batch._tensor_bytes(t, what, batch.ctx.device, rows)
    if tuple(t.shape)[1] != row_len:
        raise ValueError(f"{what} must have rows of 32 * n_points = {row_len} bytes, got {tuple(t.shape)[1]}")
    return addr, _stride(stride, row_len)


def _ordered(batch, t, call, both_ways):
    """Run `call` with the batch's stream waiting for the tensor's current stream, and (both_ways) that stream then waiting for
    the batch's kernels, as Batch.upload_tensors and Batch.finish_into order them"""
    from .verifier import _cuda_of
    cuda = _cuda_of(t, "the tensor's module has no cuda streams to order the hints by")
    current, mine = cuda.current_stream(t.device), batch.stream
    ordered = current.cuda_stream != mine
    if ordered:
        batch_stream = cuda.ExternalStream(mine, device=t.device)
        before = cuda.Event()
        before.record(current)
        batch_stream.wait_event(before)
    call()
    if ordered and both_ways:
        after = cuda.Event()
        after.record(batch_stream)
        current.wait_event(after)


def set_hints_tensor(batch, t):
    """set_hints_device from a tensor [n, 32 Np] of uint8 on the batch's device, row stride a multiple of 16.  The batch's stream
    waits, on the device, for the tensor's current stream; the rows are copied into the batch by a kernel enqueued here, and the
    batch keeps the tensor referenced until the next set_hints_tensor or finish()."""
    addr, stride = _rows_tensor(batch, t, int(batch.n), "the hints")
    if not batch.n:
        return set_hints_device(batch, None, stride)
    _ordered(batch, t, lambda: set_hints_device(batch, addr, stride), False)
    batch._keep = (getattr(batch, "_keep", None), t)   # (beside upload_tensors' inputs: the copy kernel may not have run yet)


def hints(batch, first=0, count=None):
    """The canonical y of the points of proofs [first, first + count) of the last launch -> count * Np * 32 bytes, zeros for a point
    that did not decode (h2v_batch_hints; waits for the batch's stream)"""
    first, count = _range(batch, first, count)
    if not count:
        return b""
    buf = ctypes.create_string_buffer(max(count * _n_points(batch) * 32, 1))
    _lib.check(_library().h2v_batch_hints(batch._h, first, count, buf))
    return buf.raw[:count * _n_points(batch) * 32]


def hints_device(batch, first, count, addr, row_stride):
    """hints() into device memory, as an address: row j at addr + j * row_stride, by one kernel on the batch's stream, no host wait
    (h2v_batch_hints_device)"""
    from .verifier import _address
    first, count = _range(batch, first, count)
    row_stride = _stride(row_stride, _n_points(batch) * 32)
    addr = _address(addr, "the hints' address", needed=count > 0)
    _lib.check(_library().h2v_batch_hints_device(batch._h, first, count, c_vp(addr), row_stride))


def hints_into(batch, t, first=0, count=None):
    """hints() into a tensor [count, 32 Np] of uint8 on the batch's device, row stride a multiple of 16.  The batch's stream first
    waits for the tensor's current stream, and that stream then waits, on the device, for the copy: work queued on it afterwards
    sees the rows.  The host waits for nothing."""
    first, count = _range(batch, first, count)
    addr, stride = _rows_tensor(batch, t, count, "the hints' tensor")
    if not count:
        return
    _ordered(batch, t, lambda: hints_device(batch, first, count, addr, stride), True)


def hint_stats(batch):
    """-> (n_points, n_hinted, n_missed) of the last launch (h2v_batch_hint_stats; waits for the batch's stream): n * Np; the same
    when the launch had hints, else 0; the hints that were not used"""
    vals = [c_sz(0) for _ in range(3)]
    _lib.check(_library().h2v_batch_hint_stats(batch._h, *[ctypes.byref(v) for v in vals]))
    return tuple(v.value for v in vals)
