"""Feed a launched staged Batch to a resident Accumulator without a host wait: ctypes binding of include/h2v_feed.h, behind
Accumulator.feed, .settle and .pending.

Accumulator.process_batch takes a FINISHED batch and returns with the accumulator's stream idle: two host waits per launch.  feed()
is the same operation enqueued —

  acc.feed(batch)      the groups of the batch's last launch as legs, behind the launch, on the device; waits for nothing, and the
                       batch may be uploaded again at once
  acc.settle()         waits for the accumulator's stream once, commits counters and journal entries of every feed since, and
                       -> [(rc, n_proofs, n_failed)] per feed since the last settle(); rc is 0, or BadArgument for a feed that was
                       dropped on the device (a draw >= r in a tail uploaded from device memory: the points keep their value, the
                       feed's n proofs count as processed and failed)
  acc.pending          (feeds not settled, feeds not reported)

feed(b); settle() equals process_batch(b) after a host finish of the same launch, bit for bit (include/h2v_feed.h has the definition,
the ordering and the soundness argument).  Every other Accumulator method settles first; the reports wait for the next settle().
"""
import ctypes

from . import _lib

c_vp, c_sz, c_int = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int

# the symbols include/h2v_feed.h declares: (restype, argtypes).  A table of its own beside _lib.SIGNATURES, which mirrors include/h2v.h
SIGNATURES = {
    "h2v_accumulator_feed_batch": (c_int, [c_vp, c_vp]),
    "h2v_accumulator_pending": (c_int, [c_vp, ctypes.POINTER(c_sz), ctypes.POINTER(c_sz)]),
    "h2v_accumulator_settle": (c_int, [c_vp, c_sz, ctypes.POINTER(c_sz), ctypes.POINTER(c_int), ctypes.POINTER(c_sz), ctypes.POINTER(c_sz)]),
}
FEED_MAX_PENDING = 64        # include/h2v_feed.h H2V_FEED_MAX_PENDING
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


def feed(acc, batch):
    """h2v_accumulator_feed_batch: the Python-side refusals first (none of them needs the library), then the call.  The accumulator
    remembers the feed's group count for the journal's `_inputs` (settle)."""
    from .verifier import Batch
    if not isinstance(batch, Batch):
        raise TypeError("feed takes a Batch")
    if acc._keep_inputs:
        raise ValueError("feed on an Accumulator with keep_inputs=True: retained inputs are host bytes and a Batch has none; "
                         "use Batch.identify() on the resident batch to name the proofs of a failing group")
    if not acc._h or not batch._h:
        raise ValueError("the accumulator or the batch is closed")
    if acc._feed_reports and pending(acc)[1] >= FEED_MAX_PENDING:
        # (reports this object took over at an implicit settle count like the library's own)
        raise _lib.H2VError(-19, f"h2v_accumulator_feed_batch: {FEED_MAX_PENDING} feeds wait for settle() (H2V_FEED_MAX_PENDING)")
    _lib.check(_library().h2v_accumulator_feed_batch(acc._h, batch._h))
    if int(getattr(batch, "n", 0)):   # (an upload of no proofs enqueues nothing and leaves no report)
        acc._fed_groups.append(int(batch.groups))


def pending(acc):
    """-> (n_unsettled, n_unreported) of h2v_accumulator_pending: host state only"""
    if not acc._h:
        raise ValueError("the accumulator is closed")
    u, r = c_sz(0), c_sz(0)
    _lib.check(_library().h2v_accumulator_pending(acc._h, ctypes.byref(u), ctypes.byref(r)))
    return u.value, r.value + len(acc._feed_reports)   # (the reports this object took over at an implicit settle wait for settle() too)


def collect(acc):
    """h2v_accumulator_settle, its reports moved to acc._feed_reports: what settle() hands out and what every other Accumulator method
    begins with, so that `_inputs` has the entries of the feeds the C side is about to settle.  One None per committed group."""
    if not acc._fed_groups or not acc._h:
        return
    lib = _library()
    n = c_sz(0)
    _lib.check(lib.h2v_accumulator_settle(acc._h, 0, ctypes.byref(n), None, None, None))
    cap = n.value
    rc, proofs, failed = (c_int * max(cap, 1))(), (c_sz * max(cap, 1))(), (c_sz * max(cap, 1))()
    _lib.check(lib.h2v_accumulator_settle(acc._h, cap, ctypes.byref(n), rc, proofs, failed))
    for i in range(n.value):
        groups = acc._fed_groups.pop(0)
        if rc[i] == 0 and acc._inputs:   # (journal on: the feed has left an entry per group)
            acc._inputs.extend([None] * groups)
        acc._feed_reports.append((rc[i], proofs[i], failed[i]))


def settle(acc):
    """-> [(rc, n_proofs, n_failed)] of every feed since the last settle(), in feed order"""
    if not acc._h:
        raise ValueError("the accumulator is closed")
    collect(acc)
    out, acc._feed_reports = acc._feed_reports, []
    return out
