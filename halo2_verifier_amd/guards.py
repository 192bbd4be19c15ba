"""Every proof's Guard out of a launched staged batch: ctypes binding of include/h2v_guards.h, behind Batch.guard_shape, .guards,
.guards_into and .guards_append.

A Batch runs verify_proof for all its proofs in one launch; a caller who keeps a VerificationStrategy of their own wants what
verify_proof returns, the GuardKZG of every proof: two term lists (left and right channel of its DualMSM).  After a launch they lie
resident on the GPU, and one kernel gathers any range of them

  guards(batch, first, count)          into host memory -> one dict per proof, as Context.guard_msm returns it, plus mult and status
  guards_into(batch, ..., tensors)     into device memory (tensors or raw addresses), without a host wait
  guards_append(batch, left, right)    behind the end of two resident MSMKZG objects, without a byte in between

Term t of proof first + j lies at index j * T + t of a channel (T = T_L or T_R of guard_shape).  A scalar is the Guard's own times
mult, the product of the draws behind the proof inside its group: the terms are what the reference's msm_accumulator holds for the
proof once its group has been processed, and with unit draws the raw GuardKZG.  SHPLONK: the reference's term order; GWC: a
commitment opened at several points occurs once, at its first appearance, with its scalars summed (sum-equal to the reference's
per-query list, which Context.guard_msm keeps returning).  A proof with a non-zero status has zero scalars under all-zero bases.
"""
import ctypes

from . import _lib

c_vp, c_sz, c_int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int

# the symbols include/h2v_guards.h declares: (restype, argtypes).  A table of its own beside _lib.SIGNATURES, which mirrors include/h2v.h
SIGNATURES = {
    "h2v_batch_guard_shape": (c_int, [c_vp, ctypes.POINTER(c_sz), ctypes.POINTER(c_sz)]),
    "h2v_batch_guards_device": (c_int, [c_vp, c_sz, c_sz, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "h2v_batch_guards": (c_int, [c_vp, c_sz, c_sz, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.POINTER(c_int)]),
    "h2v_batch_guards_append": (c_int, [c_vp, c_sz, c_sz, c_vp, c_vp, ctypes.POINTER(c_sz)]),
}
MAX_CALL_TERMS = 1 << 31     # one call gathers fewer terms than this per channel
OUTPUTS = ("left_scalars", "left_bases", "right_scalars", "right_bases", "mult", "status")
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


def _range(batch, first, count):
    """(first, count) of a call, checked against the batch's upload of batch.n proofs; count None: to the end"""
    from .verifier import _integer
    n = int(getattr(batch, "n", 0))
    first = _integer(first, "first")
    if first > n:
        raise ValueError(f"first = {first} lies outside the upload of {n} proofs")
    count = n - first if count is None else _integer(count, "count")
    if count > n - first:
        raise ValueError(f"proofs [{first}, {first + count}) lie outside the upload of {n} proofs")
    return first, count


def guard_shape(batch):
    """-> (T_L, T_R): the terms of a proof's left and right channel under the plan of the batch's upload (h2v_batch_guard_shape)"""
    tl, tr = c_sz(0), c_sz(0)
    _lib.check(_library().h2v_batch_guard_shape(batch._h, ctypes.byref(tl), ctypes.byref(tr)))
    return tl.value, tr.value


def output_sizes(count, shape):
    """the bytes of the six outputs of a call over `count` proofs, in the order of OUTPUTS"""
    tl, tr = shape
    if count * max(tl, tr, 1) >= MAX_CALL_TERMS:
        raise ValueError(f"{count} proofs of {max(tl, tr)} terms are 2^31 terms or more: take the range in pieces")
    return (32 * count * tl, 64 * count * tl, 32 * count * tr, 64 * count * tr, 32 * count, 4 * count)


def guards(batch, first=0, count=None):
    """The Guards of proofs [first, first + count) of the last launch (h2v_batch_guards: one kernel, one copy, one synchronise of the
    batch's stream) -> one dict per proof with right_scalars, left_scalars (32-byte strings), right_bases, left_bases (64-byte x | y,
    zeros = the identity) as Context.guard_msm returns them, and mult (32 bytes) and status (int)."""
    first, count = _range(batch, first, count)
    if not count:
        return []
    tl, tr = shape = guard_shape(batch)
    bufs = [ctypes.create_string_buffer(max(size, 1)) for size in output_sizes(count, shape)[:5]]
    st = (c_int * count)()
    _lib.check(_library().h2v_batch_guards(batch._h, first, count, *bufs, st))
    ls, lb, rs, rb, mu = (b.raw for b in bufs)
    cut = lambda raw, size, lo, k: [raw[size * (lo + i):size * (lo + i + 1)] for i in range(k)]
    return [dict(right_scalars=cut(rs, 32, j * tr, tr), right_bases=cut(rb, 64, j * tr, tr), left_scalars=cut(ls, 32, j * tl, tl),
                 left_bases=cut(lb, 64, j * tl, tl), mult=mu[32 * j:32 * j + 32], status=st[j]) for j in range(count)]


def guards_device(batch, first, count, left_scalars=None, left_bases=None, right_scalars=None, right_bases=None, mult=None, status=None):
    """h2v_batch_guards_device with raw device addresses (None = not wanted), each 16-byte aligned: device work on the batch's stream
    only; the host waits for nothing."""
    from .verifier import _address
    first, count = _range(batch, first, count)
    addrs = [_address(v, what + "'s address", "an integer address or None", positive=True)
             for v, what in zip((left_scalars, left_bases, right_scalars, right_bases, mult, status), OUTPUTS)]
    _lib.check(_library().h2v_batch_guards_device(batch._h, first, count, *[c_vp(a) for a in addrs]))


def guards_into(batch, first=0, count=None, left_scalars=None, left_bases=None, right_scalars=None, right_bases=None, mult=None, status=None):
    """guards() into device memory (h2v_batch_guards_device).  Each output is None (not wanted), a contiguous tensor on the batch's
    device — uint8 with 32 * count * T_L, 64 * count * T_L, 32 * count * T_R, 64 * count * T_R and 32 * count elements, status int32
    with count — or an integer device address, which is taken as given.  With tensors the batch's stream first waits for the
    tensors' current stream, and that stream then waits, on the device, for the batch's kernels, as Batch.finish_into orders them.
    The host waits for nothing; the outputs are the caller's to keep alive until that work has run."""
    from .verifier import Batch, _cuda_of
    first, count = _range(batch, first, count)
    given = (left_scalars, left_bases, right_scalars, right_bases, mult, status)
    if all(v is None for v in given):
        raise ValueError("guards_into: no output given")
    tensors = [v for v in given if v is not None and hasattr(v, "data_ptr")]
    addrs = list(given)
    if tensors:
        sizes = output_sizes(count, guard_shape(batch))
        for k, (v, what) in enumerate(zip(given, OUTPUTS)):
            if v is not None and hasattr(v, "data_ptr"):
                dtypes = ("int32",) if what == "status" else ("uint8",)
                addrs[k] = Batch._tensor_words(v, what, batch.ctx.device, dtypes, sizes[k] // (4 if what == "status" else 1))[0]
    if not count:
        return
    ordered = False
    if tensors:
        cuda = _cuda_of(tensors[0], "the tensors' module has no cuda streams to order the results by")
        current, mine = cuda.current_stream(tensors[0].device), batch.stream
        ordered = current.cuda_stream != mine
        if ordered:
            batch_stream = cuda.ExternalStream(mine, device=tensors[0].device)
            before = cuda.Event()
            before.record(current)
            batch_stream.wait_event(before)
    guards_device(batch, first, count, *addrs)
    if ordered:
        after = cuda.Event()
        after.record(batch_stream)
        current.wait_event(after)


def guards_append(batch, left=None, right=None, first=0, count=None):
    """The left terms of proofs [first, first + count) behind the end of `left` and their right terms behind the end of `right`
    (MSMKZG objects of the batch's device and params; either may be None), in the objects' own form (h2v_batch_guards_append).
    -> the number of proofs of the range with a non-zero status (their terms are zero terms on the identity).  A call that raises
    leaves both objects as they were."""
    from .verifier import MSMKZG
    first, count = _range(batch, first, count)
    for m, what in ((left, "left"), (right, "right")):
        if m is not None and not isinstance(m, MSMKZG):
            raise TypeError(f"{what} must be an MSMKZG or None, got {type(m).__name__}")
    if left is not None and left is right:
        raise ValueError("left and right are the same object")
    if count and (left is not None or right is not None):
        for m, what, terms in zip((left, right), ("left", "right"), guard_shape(batch)):
            if m is not None and len(m) + count * terms > MSMKZG.MAX_TERMS:
                raise ValueError(f"{what} holds {len(m)} terms: {count * terms} more are more than 2^24 terms in one object")
    failed = c_sz(0)
    _lib.check(_library().h2v_batch_guards_append(batch._h, first, count, left._handle() if left is not None else None,
                                                  right._handle() if right is not None else None, ctypes.byref(failed)))
    return failed.value
