"""Host-side mirror of the reference's verifier surface over the C ABI (include/h2v.h).

Reference names kept (halo2_verifier/src/lib.rs:29-49, poly/kzg/strategy.rs:55-181,
poly/kzg/commitment.rs:22-29, plonk/vk.rs:16-26, helpers.rs:7-19, plonk/mod.rs:19-32):
``verify_proof``, ``VerifyingKey``, ``ParamsKZG``, ``SerdeFormat``, ``AccumulatorStrategy``,
``SingleStrategy``, and the ``Error`` variants as ``PlonkError``.  All arithmetic happens in the HIP
library; this file only marshals bytes.
"""
import collections
import contextlib
import ctypes
import enum
import numbers
import struct
import sys

from . import _lib
from . import feed as _feed
from ._lib import H2VError, check


class SerdeFormat(enum.IntEnum):  # helpers.rs:7-19
    Processed = 0
    RawBytes = 1
    RawBytesUnchecked = 2


class PlonkError(enum.IntEnum):  # plonk/mod.rs:19-32 (+ the reference's panics as one extra code)
    Ok = 0
    InvalidInstances = -1
    ConstraintSystemFailure = -2
    BoundsFailure = -3
    Opening = -4
    Transcript = -5
    InstanceTooLarge = -6
    ReferencePanic = -7


class MultiOpen(enum.IntEnum):  # the `V: Verifier` parameter of verify_proof (lib.rs:35): VerifierSHPLONK / VerifierGWC
    SHPLONK = 0
    GWC = 1


class TranscriptKind(enum.IntEnum):  # the `T: TranscriptRead` parameter (lib.rs:37): Blake2bRead / Keccak256Read
    Blake2b = 0
    Keccak256 = 1


class _Options(ctypes.Structure):   # h2v_options
    _fields_ = [("struct_size", ctypes.c_size_t), ("multiopen", ctypes.c_int), ("transcript", ctypes.c_int), ("circuit_instances", ctypes.c_int),
                ("instance_kernel_threshold", ctypes.c_int)]


class _Tuning(ctypes.Structure):    # h2v_tuning (debug / test): forced kernel variants, 0 = automatic
    _fields_ = [("struct_size", ctypes.c_size_t)] + [(k, ctypes.c_int) for k in (
        "frvm_streams", "frvm_lds_kb", "msm_parts", "msm_global_sort", "msm_no_term_split", "msm_window_threads", "msm_window_wpw",
        "msm_window_slots", "pairing_one_stream")]


class ParamsKZG:
    """Verifier-side KZG parameters: k, g, g2, s_g2 (poly/kzg/commitment.rs:22-29) as bytes."""

    def __init__(self, data: bytes, fmt: SerdeFormat = SerdeFormat.RawBytes):
        self.data = bytes(data)
        self.format = SerdeFormat(fmt)

    @classmethod
    def read(cls, data, fmt=SerdeFormat.RawBytes):  # Params::read uses RawBytes (commitment.rs:271-278)
        return cls(data, fmt)

    @classmethod
    def from_bytes(cls, data):  # ParamsKZG::from_bytes uses Processed (commitment.rs:226-232)
        return cls(data, SerdeFormat.Processed)

    @property
    def k(self):
        return int.from_bytes(self.data[:4], "little")

    def to_bytes(self, fmt: SerdeFormat = SerdeFormat.Processed) -> bytes:
        """ParamsKZG::write_custom / to_bytes in another SerdeFormat (kzg/commitment.rs:142-152, 215-224; to_bytes = Processed)."""
        lib = _lib.load_library()
        n = ctypes.c_size_t(0)
        check(lib.h2v_params_convert(self.data, len(self.data), int(self.format), int(fmt), None, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value)
        check(lib.h2v_params_convert(self.data, len(self.data), int(self.format), int(fmt), buf, ctypes.byref(n)))
        return buf.raw[: n.value]

    def write(self, fmt: SerdeFormat = SerdeFormat.RawBytes) -> bytes:
        return self.to_bytes(fmt)


class VerifyingKey:
    """VerifyingKey bytes in the reference's format (plonk/vk.rs:41-115)."""

    def __init__(self, data: bytes, fmt: SerdeFormat = SerdeFormat.RawBytes):
        self.data = bytes(data)
        self.format = SerdeFormat(fmt)

    @classmethod
    def read(cls, data, fmt):
        return cls(data, fmt)

    from_bytes = read

    LAYOUT_WRITER, LAYOUT_READER = 0, 1

    def to_bytes(self, fmt: SerdeFormat, layout: int = 0) -> bytes:
        """VerifyingKey::write / to_bytes (plonk/vk.rs:41-64, 118-123) in `fmt`.  layout: LAYOUT_WRITER = exactly what the reference's
        writer emits; LAYOUT_READER = what its reader consumes — they differ for lookup / shuffle arguments of more than one
        expression pair (include/h2v.h, h2v_vk_convert)."""
        lib = _lib.load_library()
        n = ctypes.c_size_t(0)
        check(lib.h2v_vk_convert(self.data, len(self.data), int(self.format), int(fmt), int(layout), None, ctypes.byref(n)))
        buf = ctypes.create_string_buffer(n.value)
        check(lib.h2v_vk_convert(self.data, len(self.data), int(self.format), int(fmt), int(layout), buf, ctypes.byref(n)))
        return buf.raw[: n.value]

    write = to_bytes


def _scalar32(v) -> bytes:
    """One field element at the boundary: 32 little-endian bytes.  The C side reads exactly 32 bytes per scalar, so a
    shorter bytes object would make it read past the Python buffer: reject it here."""
    if isinstance(v, (bytes, bytearray, memoryview)):
        if len(v) != 32:
            raise ValueError(f"a scalar given as bytes must be exactly 32 bytes, got {len(v)}")
        return bytes(v)
    v = int(v)
    if v < 0 or v >> 256:
        raise ValueError("a scalar given as an integer must be in [0, 2^256)")
    return v.to_bytes(32, "little")


def _flatten_instances(instances):
    """instances: list (columns) of lists of 32-byte scalars (or ints) -> (flat bytes, col_lens)"""
    flat = bytearray()
    lens = []
    for col in instances:
        lens.append(len(col))
        for v in col:
            flat += _scalar32(v)
    return bytes(flat), lens


def _sizes(values):
    """values as a size_t array (of at least one element)"""
    values = list(values)
    return (ctypes.c_size_t * max(len(values), 1))(*values)


MAX_GROUPS = 512   # groups of one launch: half of the MSM's problems per launch (MSM_MAX_PROBLEMS / 2)


def _group_sizes(sizes, what="group"):
    """The sizes of the groups of a launch (or of the batches of a call), checked: integers >= 1.  -> list of ints"""
    out = []
    for v in sizes:
        if isinstance(v, bool) or not isinstance(v, numbers.Integral):
            raise TypeError(f"a {what} size must be an integer, got {type(v).__name__}")
        if v < 1:
            raise ValueError(f"every {what} holds at least one proof, got a size of {int(v)}")
        out.append(int(v))
    return out


def _rand_bytes(rand, n):
    """The draws of a one-shot call as n 32-byte scalars, or None (the library draws them)."""
    if rand is None:
        return None
    if len(rand) != n:
        raise ValueError(f"rand must hold one scalar per proof ({n}), got {len(rand)}")   # the C side reads n * 32 bytes
    return b"".join(_scalar32(r) for r in rand)


def _channel(side, what=""):
    """One channel of a DualMSM given as (scalars, bases) -> (scalar bytes, base bytes, n), the triple the seeded entry points and
    h2v_accumulator_add_msm take; everything the C side indexes is checked here.  what: "seed " in the messages of a seed's channels."""
    scalars, bases = side
    scalars, bases = list(scalars), list(bases)
    if len(scalars) != len(bases):
        raise ValueError(f"{what}scalars and bases differ in length")   # MSMKZG keeps them parallel (msm.rs:17-24)
    if any(not isinstance(b, (bytes, bytearray, memoryview)) or len(b) != 64 for b in bases):
        raise ValueError(f"every {what}base must be 64 bytes (x | y)")
    return b"".join(_scalar32(x) for x in scalars), b"".join(bytes(b) for b in bases), len(scalars)


def _seed_sides(seed):
    """The two channels of a seed DualMSM, ((left_scalars, left_bases), (right_scalars, right_bases)), as the six arguments the seeded
    entry points take"""
    sides = [_channel(side, "seed ") for side in seed]
    if len(sides) != 2:
        raise ValueError("a seed is (left, right)")
    return sides[0] + sides[1]


def _guard_sides(guard):
    """A Guard — ((left_scalars, left_bases), (right_scalars, right_bases)), or the dict Context.guard_msm returns — as (left, right)"""
    if isinstance(guard, dict):
        return (guard["left_scalars"], guard["left_bases"]), (guard["right_scalars"], guard["right_bases"])
    sides = tuple(guard)
    if len(sides) != 2:
        raise ValueError("a guard is (left, right)")
    return sides


def _guards_args(guards):
    """Guards as the arguments h2v_accumulator_process_guards / h2v_guards_check_each take in a row: (n, left_counts, right_counts,
    left_scalars32, left_bases64, right_scalars32, right_bases64), the terms of all guards back to back in guard order; everything the
    C side indexes is checked here (_channel)."""
    counts, sc, bs = ([], []), ([], []), ([], [])
    n = 0
    for i, guard in enumerate(guards):
        n += 1
        for side, ch in enumerate(_guard_sides(guard)):
            s, b, k = _channel(ch, f"guard {i}: ")
            counts[side].append(k); sc[side].append(s); bs[side].append(b)
    return (n, _sizes(counts[0]), _sizes(counts[1]), b"".join(sc[0]), b"".join(bs[0]), b"".join(sc[1]), b"".join(bs[1]))


def _points(buf, k):
    """k 64-byte points (x | y) out of a result buffer"""
    raw = buf.raw
    return [raw[64 * i:64 * i + 64] for i in range(k)]


class _Marshalled(collections.namedtuple("_Marshalled", "n proofs proof_lens instances shapes ncols keys keep")):
    """What _marshal_batch returns: proof pointers and lengths, instance pointers, the per-proof column lengths [n][ncols], the column
    count of every key, the key index of every proof and the keep-alive list."""

    @property
    def head(self):
        """(n, proofs, proof_lens, instances32): the arguments every one-shot entry point takes in a row"""
        return self[:4]

    @property
    def uniform(self):
        return all(l == self.shapes[0] for l in self.shapes)

    def shape0(self):
        """The column lengths of a call whose proofs share one instance shape: proof 0's, or empty columns for no proofs."""
        return _sizes(self.shapes[0] if self.shapes else [0] * self.ncols[0])

    def per_proof(self):
        """The column lengths proof by proof."""
        return _sizes(v for l in self.shapes for v in l)


def _marshal_batch(contexts, proofs, instances, key_of_proof=None):
    """Pointer arrays for the one-shot calls.  Everything the C side will index is checked here: one instance list per proof,
    proofs are bytes, key indices are in range, every scalar is 32 bytes, the proofs of a key have one column count.  Proof i
    belongs to contexts[key_of_proof[i]] (None: to contexts[0]).  -> _Marshalled."""
    n = len(proofs)
    if len(instances) != n:
        raise ValueError(f"{n} proofs but {len(instances)} instance lists: verify_proof takes one per proof (lib.rs:33-49)")
    for p in proofs:
        if not isinstance(p, (bytes, bytearray)):
            raise TypeError("proofs must be bytes")
    if key_of_proof is None:
        keys = [0] * n
    else:
        keys = [int(k) for k in key_of_proof]
        for k in keys:
            if not 0 <= k < len(contexts):
                raise ValueError(f"key index {k} out of range for {len(contexts)} contexts")
    flats, shapes = [], []
    for inst in instances:
        f, l = _flatten_instances(inst)
        flats.append(f)
        shapes.append(l)
    pairs = set(zip(keys, map(len, shapes)))   # (key, column count)
    ncols = dict(pairs)
    if len(ncols) != len(pairs):
        raise ValueError("all proofs of one VerifyingKey must have the same number of instance columns")
    ncols = [ncols[k] if k in ncols else c.proof_shape()["n_instance_columns"] for k, c in enumerate(contexts)]
    PA = ctypes.c_char_p * max(n, 1)
    pa = PA(*[bytes(p) for p in proofs]) if n else PA()
    ia = PA(*flats) if n else PA()
    return _Marshalled(n, pa, _sizes(len(p) for p in proofs), ia, shapes, ncols, keys, flats)


class _Results:
    """The outputs of a one-shot call over n proofs: statuses, verdict, the two evaluated channels, and for the identifying entry points
    the number of range checks and the seed's own verdict."""

    def __init__(self, n):
        self.n = n
        self.st = (ctypes.c_int * max(n, 1))()
        self.ok = ctypes.c_int(0)
        self.left, self.right = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        self.checks, self.seed_ok = ctypes.c_size_t(0), ctypes.c_int(1)

    @property
    def statuses(self):
        return list(self.st)[:self.n]

    def result(self):
        """(batch_ok, statuses, left_xy, right_xy)"""
        return bool(self.ok.value), self.statuses, self.left.raw, self.right.raw


def _keyed_args(contexts, key_of_proof, proofs, instances, rand, bare_context=False):
    """The arguments h2v_verify_batch_keys, h2v_verify_batch_keys_identify and h2v_accumulator_process share, from the contexts to the
    draws, checked -> (tuple of arguments, contexts, key_of_proof or None).  bare_context: a single Context with key_of_proof=None is
    accepted as the one-key form (Accumulator.process), and the draws are refused before the proofs are looked at, as that call always did."""
    one_key = bare_context and isinstance(contexts, Context)
    if one_key:
        if key_of_proof is not None:
            raise ValueError("a single Context takes key_of_proof=None")
        contexts = [contexts]
    else:
        contexts = list(contexts)
        if bare_context and key_of_proof is None:
            raise ValueError("a list of contexts takes one key index per proof")
    n = len(proofs)
    if (not one_key and len(key_of_proof) != n) or len(instances) != n:
        raise ValueError(f"{n} proofs need {n} key indices and {n} instance lists, got {n if one_key else len(key_of_proof)} and {len(instances)}")
    if not contexts:
        raise ValueError("at least one context")
    rb = _rand_bytes(rand, n) if bare_context else None
    m = _marshal_batch(contexts, proofs, instances, key_of_proof)
    if not bare_context:
        rb = _rand_bytes(rand, n)
    ka = (ctypes.c_uint32 * max(n, 1))(*m.keys)
    ca = (ctypes.c_void_p * len(contexts))(*[c._h.value for c in contexts])
    return (ca, len(contexts), ka, *m.head, _sizes(m.ncols), m.per_proof(), rb), contexts, None if one_key else m.keys


def _hinted_keyed(entry, handle, contexts, key_of_proof, proofs, instances, rand, hint_rows, outs, bare_context=False):
    """A keyed call with hint rows (include/h2v_hint_rows.h: hint_rows after proof_lens, the counters last): the rows are checked before
    anything else -> (the contexts, the key indices or None, (points, hinted, missed))"""
    from . import hints
    one_key = bare_context and isinstance(contexts, Context)
    ctx_list = [contexts] if one_key else list(contexts)
    keys = [0] * len(proofs) if one_key or key_of_proof is None else [int(k) for k in key_of_proof]
    if any(not 0 <= k < len(ctx_list) for k in keys):
        raise ValueError(f"key index out of range for {len(ctx_list)} contexts")
    rows = hints.call_rows(ctx_list, keys, hint_rows)
    args, contexts, keys = _keyed_args(contexts, key_of_proof, proofs, instances, rand, bare_context)
    stats = hints.stats_out()
    head = args[:6] + (rows,) + args[6:]           # (ctxs, n_keys, key_of_proof, n, proofs, proof_lens | hint_rows | instances32, ...)
    check(getattr(hints._library(), entry)(*((handle,) if handle is not None else ()), *head, *outs, stats))
    return contexts, keys, tuple(stats)


class Context:
    """ParamsKZG + VerifyingKey resident on one GPU (h2v_ctx)."""

    def __init__(self, params: ParamsKZG, vk: VerifyingKey = None, device: int = 0, multiopen=MultiOpen.SHPLONK,
                 transcript=TranscriptKind.Blake2b, circuit_instances: int = 1, instance_kernel_threshold: int = 0):
        """circuit_instances = len(instances) of the reference's verify_proof (`instances: &[&[&[Fr]]]`, lib.rs:43): how many
        circuit instances share one proof transcript.  With M > 1 the `instances` of a proof is the list of its M x columns,
        instance by instance."""
        self._lib = _lib.load_library()
        self._h = ctypes.c_void_p()
        vkb = vk.data if vk is not None else None
        opts = _Options(ctypes.sizeof(_Options), int(multiopen), int(transcript), int(circuit_instances), int(instance_kernel_threshold))
        self.circuit_instances = int(circuit_instances)
        check(self._lib.h2v_ctx_create_ex(params.data, len(params.data), int(params.format), vkb, len(vkb) if vkb else 0,
                                          int(vk.format) if vk is not None else 0, device, ctypes.byref(opts), ctypes.byref(self._h)))
        self.params, self.vk, self.device = params, vk, device

    def _adopt(self, obj):
        """A batch or an accumulator that lives on this context: close() closes it first"""
        if not hasattr(self, "_batches"):
            import weakref
            self._batches = weakref.WeakSet()
        self._batches.add(obj)

    def close(self):
        if self._h:
            for b in list(getattr(self, "_batches", ())):   # h2v_ctx_destroy: the context's batches go first
                b.close()
            self._lib.h2v_ctx_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_tuning(self, **fields):
        """Debug / test (h2v_ctx_set_tuning): force kernel variants the library otherwise chooses from the launch shape, e.g.
        set_tuning(frvm_streams=2, msm_window_slots=3).  No arguments = back to automatic.  Not synchronised with launches in
        flight: call while the context is idle."""
        if not fields:
            check(self._lib.h2v_ctx_set_tuning(self._h, None))
            return
        t = _Tuning(ctypes.sizeof(_Tuning))
        for k, val in fields.items():
            if k == "struct_size" or not hasattr(t, k):
                raise ValueError(f"unknown tuning field {k!r}")
            setattr(t, k, int(val))
        check(self._lib.h2v_ctx_set_tuning(self._h, ctypes.byref(t)))

    # -- MSMKZG::eval (poly/kzg/msm.rs:81-86)
    def msm_g1(self, scalars, bases):
        """scalars: iterable of ints / 32-byte LE; bases: iterable of 64-byte x|y. -> 64-byte x|y (zeros = identity)"""
        sb = b"".join(_scalar32(s) for s in scalars)
        bases = list(bases)
        if any(len(b) != 64 for b in bases):
            raise ValueError("every base must be 64 bytes (x | y)")
        bb = b"".join(bases)
        n = len(sb) // 32
        if len(bb) != 64 * n:
            raise ValueError("scalars and bases differ in length")  # best_multiexp asserts equal lengths (arithmetic.rs:103)
        out = ctypes.create_string_buffer(64)
        ident = ctypes.c_int(0)
        check(self._lib.h2v_msm_g1(self._h, sb, bb, n, out, ctypes.byref(ident)))
        return out.raw

    # -- DualMSM::check (poly/kzg/msm.rs:185-203)
    def pairing_check(self, left_xy: bytes, right_xy: bytes) -> bool:
        ok = ctypes.c_int(0)
        if len(left_xy) != 64 or len(right_xy) != 64:
            raise ValueError("points are 64 bytes (x | y)")
        check(self._lib.h2v_pairing_check(self._h, left_xy, right_xy, ctypes.byref(ok)))
        return bool(ok.value)

    # -- n x DualMSM::check: SingleStrategy at the trait seam (poly/kzg/strategy.rs:164-176)
    def guards_check_each(self, guards):
        """One pairing verdict per Guard (h2v_guards_check_each), the Guards as a CPU verify_proof hands them over: each
        ((left_scalars, left_bases), (right_scalars, right_bases)) or the dict guard_msm returns.  -> [bool]: e(L_i, s_g2) e(R_i, -g2) == 1
        over guard i's own evaluated channels.  A malformed term raises H2VError naming the guard and the side."""
        args = _guards_args(guards)
        ok = (ctypes.c_int * max(args[0], 1))()
        check(self._lib.h2v_guards_check_each(self._h, *args, ok))
        return [bool(v) for v in ok][:args[0]]

    def proof_shape(self):
        vals = [ctypes.c_size_t(0) for _ in range(5)]
        check(self._lib.h2v_ctx_proof_shape(self._h, *[ctypes.byref(v) for v in vals]))
        keys = ("proof_len", "n_points", "n_scalars", "n_right_terms", "n_instance_columns")
        return dict(zip(keys, (v.value for v in vals)))

    # -- N x verify_proof + AccumulatorStrategy::finalize
    def verify_batch(self, proofs, instances, rand=None, seed=None, hints=None):
        """proofs: list of bytes; instances: per proof, list of columns of scalars (column lengths may differ from proof to
        proof, as N independent verify_proof calls allow); rand: list of n ints/bytes or None.
        seed: an existing accumulator to start from — AccumulatorStrategy::with (kzg/strategy.rs:75-78) — as
        ((left_scalars, left_bases), (right_scalars, right_bases)): scalars ints / 32-byte strings, bases 64-byte x | y.
        hints: per proof its hint row (hints.for_proofs: n_points * 32 bytes) or None (h2v_verify_batch_keys_hinted; not with a seed): the
        same results sooner; (points, hinted points, hinted points missed) are kept in self.last_hint_stats.
        Returns (batch_ok, statuses, left_xy, right_xy)."""
        if hints is not None:
            if seed is not None:
                raise ValueError("a seeded batch takes no hints")
            r = _Results(len(proofs))
            _, _, self.last_hint_stats = _hinted_keyed("h2v_verify_batch_keys_hinted", None, [self], [0] * len(proofs), proofs, instances, rand, hints,
                                                       (r.st, ctypes.byref(r.ok), r.left, r.right))
            return r.result()
        m = _marshal_batch([self], proofs, instances)
        rb = _rand_bytes(rand, m.n)
        r = _Results(m.n)
        outs = (r.st, ctypes.byref(r.ok), r.left, r.right)
        if seed is not None:
            if not m.uniform:
                raise ValueError("a seeded batch takes one instance shape")
            sides = _seed_sides(seed)
            check(self._lib.h2v_verify_batch_seeded(self._h, *m.head, m.ncols[0], m.shape0(), rb, *sides, *outs))
        elif m.uniform:
            check(self._lib.h2v_verify_batch(self._h, *m.head, m.ncols[0], m.shape0(), rb, *outs))
        else:
            check(self._lib.h2v_verify_batch_shapes(self._h, *m.head, m.ncols[0], m.per_proof(), rb, *outs))
        return r.result()

    def verify_batch_identify(self, proofs, instances, rand=None, seed=None):
        """verify_batch plus the proofs that made it fail (h2v_verify_batch_identify).  Returns (batch_ok, statuses, left_xy, right_xy):
        batch_ok / left_xy / right_xy are what verify_batch returns for the same arguments, statuses[i] is what verify_each returns for
        proof i.  rand: n non-zero scalars or None.  One instance shape per call.  The number of range checks the search ran is kept in
        self.last_range_checks.
        seed: as verify_batch's (h2v_verify_batch_seeded_identify).  The seed enters no proof's check; self.last_seed_ok says whether
        the seed alone passes the pairing (True without a seed, and for an empty one)."""
        m = _marshal_batch([self], proofs, instances)
        if not m.uniform:
            raise ValueError("verify_batch_identify takes one instance shape per call")
        rb = _rand_bytes(rand, m.n)
        r = _Results(m.n)
        if seed is not None:
            sides = _seed_sides(seed)
            check(self._lib.h2v_verify_batch_seeded_identify(self._h, *m.head, m.ncols[0], m.shape0(), rb, *sides, r.st, ctypes.byref(r.ok),
                                                             ctypes.byref(r.seed_ok), r.left, r.right, ctypes.byref(r.checks)))
        else:
            check(self._lib.h2v_verify_batch_identify(self._h, *m.head, m.ncols[0], m.shape0(), rb, r.st, ctypes.byref(r.ok), r.left, r.right,
                                                      ctypes.byref(r.checks)))
        self.last_range_checks, self.last_seed_ok = r.checks.value, bool(r.seed_ok.value)
        return r.result()

    def verify_batches(self, batches, rand=None, hints=None):
        """Many AccumulatorStrategy batches of their own sizes in few launches (h2v_verify_batches).  batches: list of (proofs, instances),
        each as verify_batch takes them and none empty; one instance shape for the whole call; rand: one scalar per proof of the call, batch
        after batch, or None.  hints: one row or None per proof of the call, batch after batch (h2v_verify_batches_hinted; the counters in
        self.last_hint_stats).  Returns one (batch_ok, statuses, left_xy, right_xy) per batch: what verify_batch returns for it with its draws."""
        batches = [(list(p), list(i)) for p, i in batches]
        rows = None
        if hints is not None:
            from . import hints as hints_mod
            rows = hints_mod.call_rows([self], [0] * sum(len(p) for p, _ in batches), hints)
        for p, i in batches:
            if len(i) != len(p):
                raise ValueError(f"{len(p)} proofs but {len(i)} instance lists in one batch")
        sizes = _group_sizes((len(p) for p, _ in batches), "batch")
        m = _marshal_batch([self], [x for p, _ in batches for x in p], [x for _, i in batches for x in i])
        if not m.uniform:
            raise ValueError("verify_batches takes one instance shape per call")
        rb = _rand_bytes(rand, m.n)
        k = len(sizes)
        st = (ctypes.c_int * max(m.n, 1))()
        ok = (ctypes.c_int * max(k, 1))()
        left, right = ctypes.create_string_buffer(64 * max(k, 1)), ctypes.create_string_buffer(64 * max(k, 1))
        if rows is None:
            check(self._lib.h2v_verify_batches(self._h, k, _sizes(sizes), *m.head[1:], m.ncols[0], m.shape0(), rb, st, ok, left, right))
        else:
            stats = hints_mod.stats_out()
            check(hints_mod._library().h2v_verify_batches_hinted(self._h, k, _sizes(sizes), m.proofs, m.proof_lens, rows, m.instances, m.ncols[0], m.shape0(), rb, st,
                                                                 ok, left, right, stats))
            self.last_hint_stats = tuple(stats)
        out, at = [], 0
        for g, sz in enumerate(sizes):
            out.append((bool(ok[g]), list(st[at:at + sz]), left.raw[64 * g:64 * g + 64], right.raw[64 * g:64 * g + 64]))
            at += sz
        return out

    def verify_each(self, proofs, instances):
        m = _marshal_batch([self], proofs, instances)
        if m.uniform:
            r = _Results(m.n)
            check(self._lib.h2v_verify_each(self._h, *m.head, m.ncols[0], m.shape0(), r.st))
            return r.statuses
        # SingleStrategy proofs are independent: run every instance shape as its own call and put the statuses back in order
        out = [0] * m.n
        by_shape = {}
        for i, l in enumerate(m.shapes):
            by_shape.setdefault(tuple(l), []).append(i)
        for l, idx in by_shape.items():
            sub = self.verify_each([proofs[i] for i in idx], [instances[i] for i in idx])
            for i, v in zip(idx, sub):
                out[i] = v
        return out

    def guard_msm(self, proof, instances, cap=4096):
        f, lens = _flatten_instances(instances)
        cl = _sizes(lens)
        rs, rb = ctypes.create_string_buffer(32 * cap), ctypes.create_string_buffer(64 * cap)
        ls, lb = ctypes.create_string_buffer(32 * 64), ctypes.create_string_buffer(64 * 64)
        ch = ctypes.create_string_buffer(32 * 64)
        nr, nl, nc = ctypes.c_size_t(cap), ctypes.c_size_t(64), ctypes.c_size_t(64)
        rc = self._lib.h2v_guard_msm(self._h, proof, len(proof), f, len(lens), cl, rs, rb, ctypes.byref(nr), ls, lb, ctypes.byref(nl), ch, ctypes.byref(nc))
        if rc != 0:
            return rc, None
        split = lambda buf, sz, n: [buf.raw[sz * i:sz * (i + 1)] for i in range(n)]
        return 0, dict(right_scalars=split(rs, 32, nr.value), right_bases=split(rb, 64, nr.value), left_scalars=split(ls, 32, nl.value),
                       left_bases=split(lb, 64, nl.value), challenges=split(ch, 32, nc.value))


class _Strategy:
    def __init__(self, params: ParamsKZG):
        self.params = params
        self._items = []  # (vk, instances, proof)
        self._hints = []  # per item its hint row or None (AccumulatorStrategy)


class AccumulatorStrategy(_Strategy):
    """poly/kzg/strategy.rs:55-79,125-140: collects proofs; finalize() = one pairing for all of them."""

    def __init__(self, params, rand=None, device=0, circuit_instances=1):
        super().__init__(params)
        self.rand, self.device, self.circuit_instances = rand, device, circuit_instances
        self.seed = None
        self.left_xy = self.right_xy = None   # the evaluated channels after finalize()

    @classmethod
    def with_accumulator(cls, params, left, right, rand=None, device=0, circuit_instances=1):
        """AccumulatorStrategy::with(msm_accumulator) (kzg/strategy.rs:75-78): start from an existing DualMSM — left / right are
        (scalars, bases) term lists as MSMKZG holds them.  A finished accumulation is resumed with left = ([1], [left_xy]),
        right = ([1], [right_xy])."""
        s = cls(params, rand=rand, device=device, circuit_instances=circuit_instances)
        s.seed = (left, right)
        return s

    def finalize_identify(self) -> bool:
        """finalize() plus the proofs that made it fail (h2v_verify_batch_keys_identify), over one or several VerifyingKeys and any
        instance shapes.  Returns what finalize() returns; afterwards `statuses` holds, proof by proof in accumulation order, what
        SingleStrategy reports for it (ConstraintSystemFailure for the proofs whose own pairing fails), `left_xy` / `right_xy` the
        evaluated channels and `last_range_checks` the number of range checks the search ran.  The draws must be non-zero.
        A seeded accumulation (with_accumulator) takes proofs of one VerifyingKey and one instance shape, as finalize() does; the seed
        enters no proof's check, and `last_seed_ok` says whether the seed alone passes the pairing."""
        return self._finalize(identify=True)

    def finalize(self) -> bool:
        """One pairing for everything that was accumulated.  verify_proof takes a VK per call and one strategy may accumulate
        proofs of DIFFERENT VKs over the same params (kzg/strategy.rs:125-140 only ever sees MSMs): proofs are grouped by VK,
        every VK gets its own context, and h2v_verify_batch_keys runs them all with the draws indexed by call order over ALL
        queued proofs (proof i is scaled by the product of the draws of all later proofs, whatever their VK) into one pairing.
        left_xy / right_xy hold the evaluated channels afterwards."""
        return self._finalize(identify=False)

    @contextlib.contextmanager
    def _contexts(self):
        """The queued proofs grouped by VerifyingKey: a context per key, open for the block -> (contexts, the key index of every proof)"""
        index = {}
        for vk, _, _ in self._items:
            index.setdefault((vk.data, int(vk.format)), (len(index), vk))
        if self.seed is not None and len(index) != 1:
            raise ValueError("a seeded accumulation takes proofs of one VerifyingKey")
        ctxs = []
        try:
            for _, vk in index.values():
                ctxs.append(Context(self.params, vk, self.device, circuit_instances=self.circuit_instances))
            yield ctxs, [index[(vk.data, int(vk.format))][0] for vk, _, _ in self._items]
        finally:
            for c in ctxs:
                c.close()

    def _finalize(self, identify):
        n = len(self._items)
        if not n and not identify:
            return True  # empty DualMSM: both channels are the identity, e(0,..)e(0,..) == 1
        rand = self.rand
        if rand is not None and len(rand) != n:
            raise ValueError(f"rand must hold one scalar per accumulated proof ({n}), got {len(rand)}")
        if identify:
            self.last_seed_ok = True
            if not n:   # (as finalize())
                self.statuses, self.last_range_checks = [], 0
                return True
        proofs, instances = [p for _, _, p in self._items], [i for _, i, _ in self._items]
        with self._contexts() as (ctxs, key_of_proof):
            rows = self._hints if self.seed is None and any(h is not None for h in self._hints) else None   # (no row queued: the calls without hints)
            if not identify and len(ctxs) == 1:
                ok, _, self.left_xy, self.right_xy = ctxs[0].verify_batch(proofs, instances, rand, seed=self.seed, hints=rows)
            elif not identify:
                ok, _, self.left_xy, self.right_xy = verify_batch_keys(ctxs, key_of_proof, proofs, instances, rand, hints=rows)[:4]
            elif self.seed is not None:
                ok, self.statuses, self.left_xy, self.right_xy = ctxs[0].verify_batch_identify(proofs, instances, rand, seed=self.seed)
                self.last_range_checks, self.last_seed_ok = ctxs[0].last_range_checks, ctxs[0].last_seed_ok
            else:   # (one key too: h2v_verify_batch_keys_identify takes any instance shapes)
                ok, self.statuses, self.left_xy, self.right_xy, self.last_range_checks = verify_batch_keys_identify(ctxs, key_of_proof, proofs, instances, rand)
            return ok


class SingleStrategy(_Strategy):
    """poly/kzg/strategy.rs:83-102,164-176: one pairing per proof, checked inside verify_proof."""

    def __init__(self, params, device=0, circuit_instances=1):
        super().__init__(params)
        self.device, self.circuit_instances = device, circuit_instances


def verify_proof(params: ParamsKZG, vk: VerifyingKey, strategy, instances, proof: bytes, hints=None):
    """lib.rs:33-49.  `instances` = one circuit instance: list of columns — or, for a strategy created with circuit_instances = M,
    the M x columns of the M instances that share the transcript, instance by instance (the reference's `&[&[&[Fr]]]` flattened).
    With SingleStrategy returns None or raises H2VError(code = PlonkError); with AccumulatorStrategy returns the strategy
    (Output = Self).  hints: the proof's hint row (hints.for_proofs) for an AccumulatorStrategy, handed on at finalize(); a
    SingleStrategy, finalize_identify() and a seeded accumulation run without hints."""
    if hints is not None and not isinstance(hints, (bytes, bytearray)):
        raise TypeError("a proof's hints are one row of bytes")
    if isinstance(strategy, SingleStrategy):
        ctx = Context(params, vk, strategy.device, circuit_instances=strategy.circuit_instances)
        try:
            st = ctx.verify_each([proof], [instances])[0]
        finally:
            ctx.close()
        if st != 0:
            raise H2VError(st, PlonkError(st).name)
        return None
    strategy._items.append((vk, instances, proof))
    strategy._hints.append(hints)
    return strategy


def verify_batch(params, vk, proofs, instances, rand=None, device=0):
    ctx = Context(params, vk, device)
    try:
        return ctx.verify_batch(proofs, instances, rand)
    finally:
        ctx.close()


def verify_batch_keys(contexts, key_of_proof, proofs, instances, rand=None, hints=None):
    """N x verify_proof on ONE AccumulatorStrategy whose proofs belong to several VerifyingKeys over the same params, then
    finalize() (h2v_verify_batch_keys): contexts[k] holds key k, proof i belongs to contexts[key_of_proof[i]].  instances: per
    proof, list of columns (shapes may differ from proof to proof; every proof of a key has that key's column count).  rand: n
    draws in call order, or None.  hints: per proof its hint row — 32 bytes per point of ITS key — or None
    (h2v_verify_batch_keys_hinted); then the result has a fifth item, (points, hinted points, hinted points missed).
    Returns (batch_ok, statuses, left_xy, right_xy)."""
    r = _Results(len(proofs))
    if hints is not None:
        _, _, stats = _hinted_keyed("h2v_verify_batch_keys_hinted", None, contexts, key_of_proof, proofs, instances, rand, hints,
                                    (r.st, ctypes.byref(r.ok), r.left, r.right))
        return r.result() + (stats,)
    args, _, _ = _keyed_args(contexts, key_of_proof, proofs, instances, rand)
    check(_lib.load_library().h2v_verify_batch_keys(*args, r.st, ctypes.byref(r.ok), r.left, r.right))
    return r.result()


def verify_batch_keys_identify(contexts, key_of_proof, proofs, instances, rand=None):
    """verify_batch_keys plus the proofs that made it fail (h2v_verify_batch_keys_identify).  Same arguments as verify_batch_keys
    (several keys, per-proof instance shapes); rand: n non-zero draws in call order, or None.  Returns (batch_ok, statuses, left_xy,
    right_xy, range_checks): batch_ok / left_xy / right_xy are what verify_batch_keys returns for the same arguments, statuses[i] is what
    contexts[key_of_proof[i]].verify_each returns for proof i, range_checks the number of range checks the search ran."""
    args, _, _ = _keyed_args(contexts, key_of_proof, proofs, instances, rand)
    r = _Results(len(proofs))
    check(_lib.load_library().h2v_verify_batch_keys_identify(*args, r.st, ctypes.byref(r.ok), r.left, r.right, ctypes.byref(r.checks)))
    return r.result() + (r.checks.value,)


class Accumulator:
    """A resident AccumulatorStrategy (h2v_accumulator): two G1 points that stay on the GPU across calls.  process() feeds proofs as
    they arrive — any mix of VerifyingKeys and instance shapes over the context's params — and finalize() runs the one pairing whenever
    the caller decides (kzg/strategy.rs:125-140).  process(A); process(B); finalize() equals verify_batch_keys over A + B with the draws
    concatenated.  `context` supplies the device, the params and the pairing tables; it needs no VerifyingKey and must outlive the object.

    journal=capacity turns the leg journal on from the start (journal_begin): one entry per process / add_msm call, so that
    check_legs() names the legs whose own pairing fails and drop_legs() takes them out again.  keep_inputs=True also retains every leg's
    (contexts, key_of_proof, proofs, instances) in host memory, which lets identify() name the proofs inside a failing leg."""

    JOURNAL_MAX = 4096   # include/h2v.h H2V_ACC_JOURNAL_MAX
    _keep_inputs, _inputs = False, ()
    _fed_groups, _feed_reports = (), ()

    def __init__(self, context: Context, journal=0, keep_inputs=False):
        if not isinstance(context, Context):
            raise TypeError("Accumulator takes a Context")
        journal = self._capacity(journal)
        self.ctx, self._lib = context, context._lib
        self._h = ctypes.c_void_p()
        check(self._lib.h2v_accumulator_create(context._h, ctypes.byref(self._h)))
        context._adopt(self)
        self.last_all_ok = True
        self._keep_inputs = bool(keep_inputs)
        self._inputs = []   # with keep_inputs: one item per journal entry, None for the base and for add_msm entries
        self._fed_groups = []     # the group counts of the feeds enqueued and not settled by this object yet (feed.py)
        self._feed_reports = []   # (rc, n_proofs, n_failed) of the feeds settled on the way, for the next settle()
        if journal:
            self.journal_begin(journal)

    @classmethod
    def _capacity(cls, capacity):
        if not isinstance(capacity, int) or isinstance(capacity, bool):
            raise ValueError("the journal's capacity is an integer")
        if capacity != 0 and not 2 <= capacity <= cls.JOURNAL_MAX:
            raise ValueError(f"the journal's capacity is 0 (off) or in [2, {cls.JOURNAL_MAX}], got {capacity}")
        return capacity

    def close(self):
        if self._h:
            self._lib.h2v_accumulator_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def process(self, contexts, key_of_proof, proofs, instances, rand=None, hints=None):
        """n x verify_proof on this accumulator (h2v_accumulator_process): contexts[k] holds key k, proof i belongs to
        contexts[key_of_proof[i]]; a single Context with key_of_proof=None is the one-key form.  instances / rand as verify_batch_keys.
        hints: per proof its hint row (32 bytes per point of its key) or None (h2v_accumulator_process_hinted): the same accumulator
        sooner; the counters are kept in `last_hint_stats`.
        Returns the statuses of this call's proofs; `last_all_ok` says whether all are 0.  A call that raises H2VError leaves the
        accumulator as it was."""
        r = _Results(len(proofs))
        _feed.collect(self)
        if hints is not None:
            contexts, keys, self.last_hint_stats = _hinted_keyed("h2v_accumulator_process_hinted", self._h, contexts, key_of_proof, proofs, instances, rand, hints,
                                                                 (r.st, ctypes.byref(r.ok)), bare_context=True)
        else:
            args, contexts, keys = _keyed_args(contexts, key_of_proof, proofs, instances, rand, bare_context=True)
            check(self._lib.h2v_accumulator_process(self._h, *args, r.st, ctypes.byref(r.ok)))
        self.last_all_ok = bool(r.ok.value)
        if r.n and self._inputs:   # (journal on: the call has appended an entry)
            self._inputs.append((contexts, keys, list(proofs), list(instances)) if self._keep_inputs else None)
        return r.statuses

    def process_guards(self, guards, rand=None):
        """n x (scale by the draw, add the Guard) on this accumulator (h2v_accumulator_process_guards): the trait seam, where a CPU
        verify_proof made the Guards.  guards: each ((left_scalars, left_bases), (right_scalars, right_bases)) — scalars ints / 32-byte
        strings, bases 64-byte x | y — or the dict Context.guard_msm returns; rand: one scalar per guard, or None.  Equals process() over
        the proofs the Guards came from, with the same draws.  A call that raises H2VError leaves the accumulator as it was."""
        guards = list(guards)
        args = _guards_args(guards)
        rb = _rand_bytes(rand, args[0])
        _feed.collect(self)
        check(self._lib.h2v_accumulator_process_guards(self._h, *args, rb))
        if args[0] and self._inputs:   # (journal on: the call has appended an entry)
            self._inputs.append(("guards", guards) if self._keep_inputs else None)

    def process_batch(self, batch):
        """The groups of a finished staged Batch as legs of this accumulator, in group order (h2v_accumulator_process_batch): equals
        process() once per group over that group's proofs and draws, with the groups' sums taken from what the launch left on the GPU.
        batch: a Batch whose finish() / finish_groups() has returned, over this accumulator's device and params; it is only read and may
        be uploaded again at once.  With the journal on every group leaves an entry: check_legs() names a failing group, and
        Batch.identify() on the still-resident batch names the proofs inside it.  -> (n_proofs_added, n_failed_added).  A call that
        raises leaves the accumulator as it was."""
        if not isinstance(batch, Batch):
            raise TypeError("process_batch takes a Batch")
        if self._keep_inputs:
            raise ValueError("process_batch on an Accumulator with keep_inputs=True: retained inputs are host bytes and a Batch has none; "
                             "use Batch.identify() on the resident batch to name the proofs of a failing group")
        if not self._h or not batch._h:
            raise ValueError("the accumulator or the batch is closed")
        n, f = ctypes.c_size_t(0), ctypes.c_size_t(0)
        _feed.collect(self)
        check(self._lib.h2v_accumulator_process_batch(self._h, batch._h, ctypes.byref(n), ctypes.byref(f)))
        self.last_all_ok = f.value == 0
        if n.value and self._inputs:   # (journal on: the call has appended an entry per group)
            self._inputs.extend([None] * batch.groups)
        return n.value, f.value

    def feed(self, batch):
        """process_batch ENQUEUED (h2v_accumulator_feed_batch, include/h2v_feed.h): the groups of the last launch of `batch` — launched
        or finished — as legs of this accumulator, on the device, behind the launch.  Waits for nothing and returns nothing; the batch
        may be uploaded again at once.  Counters, journal and reports follow at settle() (or at any other method, which settles
        first).  At most feed.FEED_MAX_PENDING feeds between two settle() calls."""
        _feed.feed(self, batch)

    def settle(self):
        """Wait for the enqueued feeds and commit them (h2v_accumulator_settle) -> [(rc, n_proofs, n_failed)] of every feed since the
        last settle(), in feed order.  rc is 0, or H2V_ERR_BAD_ARGUMENT (-16) for a feed the device dropped: a draw >= r
        in a tail uploaded from device memory; the points keep their value, no journal entry appears, and both counters grow by n."""
        return _feed.settle(self)

    @property
    def pending(self):
        """(feeds not settled yet, feeds whose report settle() has not handed out yet): host state only"""
        return _feed.pending(self)

    def add_msm(self, left, right):
        """(L, R) += the two term lists evaluated, unscaled (h2v_accumulator_add_msm: AccumulatorStrategy::with on an empty accumulator,
        DualMSM::add_msm otherwise).  left / right: (scalars, bases) — scalars ints / 32-byte strings, bases 64-byte x | y."""
        l, r = _channel(left), _channel(right)
        _feed.collect(self)
        check(self._lib.h2v_accumulator_add_msm(self._h, *l, *r))
        if self._inputs:
            self._inputs.append(None)

    def add_msms(self, dual):
        """add_msm with both channels resident (h2v_accumulator_add_msms): dual is a DualMSM, or a pair (left, right) of MSMKZG objects,
        either of which may be None (empty).  The two channels are evaluated in one pooled launch and added unscaled; counters, journal
        entry and refusals are add_msm's."""
        left, right = (dual.left, dual.right) if isinstance(dual, DualMSM) else tuple(dual)
        for m in (left, right):
            if m is not None and not isinstance(m, MSMKZG):
                raise TypeError("add_msms takes a DualMSM or a pair of MSMKZG objects (or None)")
        if not self._h:
            raise ValueError("the accumulator is closed")
        _feed.collect(self)
        check(self._lib.h2v_accumulator_add_msms(self._h, left._handle() if left is not None else None, right._handle() if right is not None else None))
        if self._inputs:
            self._inputs.append(None)

    def read(self):
        """-> (left_xy, right_xy, n_proofs, n_failed): the two points as affine bytes (zeros = identity) and the counters"""
        left, right = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        n, f = ctypes.c_size_t(0), ctypes.c_size_t(0)
        check(self._lib.h2v_accumulator_read(self._h, left, right, ctypes.byref(n), ctypes.byref(f)))
        return left.raw, right.raw, n.value, f.value

    def finalize(self):
        """-> (ok, left_xy, right_xy): ok = the pairing of (L, R) passes and no processed proof failed.  The accumulator is not
        consumed: processing may go on, and finalize() may be called again."""
        ok = ctypes.c_int(0)
        left, right = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        check(self._lib.h2v_accumulator_finalize(self._h, ctypes.byref(ok), left, right))
        return bool(ok.value), left.raw, right.raw

    # -- the leg journal: find and drop failing legs
    def journal_begin(self, capacity):
        """Begin the leg journal (h2v_accumulator_journal_begin): `capacity` entries, the base included, in [2, JOURNAL_MAX]; 0 turns
        it off.  Entry 0, the base, is the accumulator as it stands; on a journaled accumulator this is a checkpoint.  Retained inputs
        are forgotten.  The points and counters do not change."""
        capacity = self._capacity(capacity)
        _feed.collect(self)
        check(self._lib.h2v_accumulator_journal_begin(self._h, capacity))
        self._inputs = [None] if capacity else []

    def check_legs(self):
        """-> [(n_proofs, n_failed, pairing_ok)] per journal entry, the base first (h2v_accumulator_check_legs): pairing_ok is the
        pairing check of the entry's own sum, every entry's side by side in one launch.  [] with the journal off."""
        n = ctypes.c_size_t(0)
        _feed.collect(self)
        check(self._lib.h2v_accumulator_check_legs(self._h, 0, ctypes.byref(n), None, None, None))
        cap = n.value
        proofs, failed, ok = (ctypes.c_size_t * max(cap, 1))(), (ctypes.c_size_t * max(cap, 1))(), (ctypes.c_int * max(cap, 1))()
        check(self._lib.h2v_accumulator_check_legs(self._h, cap, ctypes.byref(n), proofs, failed, ok))
        return [(proofs[e], failed[e], bool(ok[e])) for e in range(n.value)]

    def drop_legs(self, indices):
        """Take journal entries out again (h2v_accumulator_drop_legs): afterwards the points, the counters and the journal are those of
        an accumulator that was never given the dropped calls; later entries move down.  indices: distinct entry numbers, none 0 (the
        base stays).  An empty list rebuilds the points from the journal."""
        indices = list(indices)
        if any(not isinstance(e, int) or isinstance(e, bool) for e in indices):
            raise ValueError("entry indices are integers")
        if any(e <= 0 for e in indices):
            raise ValueError("entry indices are positive: entry 0, the base, cannot be dropped")
        if len(set(indices)) != len(indices):
            raise ValueError("an entry index given twice")
        _feed.collect(self)
        if self._inputs and any(e >= len(self._inputs) for e in indices):
            raise ValueError(f"the journal has {len(self._inputs)} entries")
        check(self._lib.h2v_accumulator_drop_legs(self._h, _sizes(indices), len(indices)))
        gone = set(indices)
        self._inputs = [x for e, x in enumerate(self._inputs) if e not in gone]

    # -- merging: one pairing for several accumulators
    MERGE_MAX = 512       # include/h2v.h H2V_ACC_MERGE_MAX
    STATE_BYTES = 152     # include/h2v.h H2V_ACC_STATE_BYTES
    STATE_MAGIC = 0x53563248   # "H2VS", include/h2v.h H2V_ACC_STATE_MAGIC
    STATE_VERSION = 1

    @staticmethod
    def pack_state(left_xy, right_xy, n_proofs, n_failed):
        """The bytes export_state() writes for these points and counters (include/h2v.h): little-endian
        [u32 magic][u32 version][u64 n_proofs][u64 n_failed][left x | y][right x | y]"""
        if len(left_xy) != 64 or len(right_xy) != 64:
            raise ValueError("a point is 64 bytes (x | y)")
        return struct.pack("<IIQQ", Accumulator.STATE_MAGIC, Accumulator.STATE_VERSION, n_proofs, n_failed) + bytes(left_xy) + bytes(right_xy)

    @staticmethod
    def unpack_state(state):
        """-> (left_xy, right_xy, n_proofs, n_failed) of a state; ValueError for a wrong length, magic or version"""
        state = bytes(state)
        if len(state) != Accumulator.STATE_BYTES:
            raise ValueError(f"a state is {Accumulator.STATE_BYTES} bytes, got {len(state)}")
        magic, version, n, f = struct.unpack_from("<IIQQ", state)
        if magic != Accumulator.STATE_MAGIC or version != Accumulator.STATE_VERSION:
            raise ValueError("a state with a wrong magic or version")
        return state[24:88], state[88:152], n, f

    def _merge_draws(self, draws, n, what):
        """(draw bytes or None, the buffer the draws used are written to), every length the C side indexes checked"""
        if n > self.MERGE_MAX:
            raise ValueError(f"a merge takes at most {self.MERGE_MAX} {what}, got {n}")
        if draws is not None and len(draws) != n:
            raise ValueError(f"draws must hold one scalar per merged accumulator ({n}), got {len(draws)}")   # the C side reads n * 32 bytes
        return (None if draws is None else b"".join(_scalar32(c) for c in draws)), ctypes.create_string_buffer(max(32 * n, 1))

    def _merged(self, n, out):
        if self._inputs:   # (journal on: the call has appended an entry per source)
            self._inputs.extend([None] * n)
        return [out.raw[32 * k: 32 * k + 32] for k in range(n)]

    def merge(self, sources, draws=None):
        """(L, R) += sum_k c_k (L_k, R_k) over the accumulators `sources`, the counters += theirs (h2v_accumulator_merge): one pairing
        for all of them afterwards.  draws: one non-zero scalar per source, or None for fresh OS draws (the sound form: the draws must
        not be known when the sources are made).  The sources are not changed; with the journal on every source leaves an entry, which
        check_legs() tests and drop_legs() takes out.  -> the draws used, 32 bytes each.  A call that raises leaves everything as it was."""
        sources = list(sources)
        if any(not isinstance(a, Accumulator) for a in sources):
            raise TypeError("merge takes Accumulators")
        if any(a is self for a in sources) or len({id(a) for a in sources}) != len(sources):
            raise ValueError("a source is the destination, or is given twice")
        if any(not a._h for a in sources):
            raise ValueError("a source is closed")
        c, out = self._merge_draws(draws, len(sources), "sources")
        for a in [self] + sources:
            _feed.collect(a)
        handles = (ctypes.c_void_p * max(len(sources), 1))(*[a._h.value for a in sources])
        check(self._lib.h2v_accumulator_merge(self._h, handles, len(sources), c, out))
        return self._merged(len(sources), out)

    def export_state(self):
        """-> the accumulator as STATE_BYTES bytes (h2v_accumulator_export_state): the counters and the two affine points, for a
        merge_states() on another device or in another process.  A state carries no SRS: the importer cannot check it."""
        out = ctypes.create_string_buffer(self.STATE_BYTES)
        check(self._lib.h2v_accumulator_export_state(self._h, out))
        return out.raw

    def merge_states(self, states, draws=None):
        """merge() over exported states (h2v_accumulator_merge_states): states is a list of STATE_BYTES-byte strings.  -> the draws used."""
        states = list(states)
        if any(not isinstance(st, (bytes, bytearray, memoryview)) or len(st) != self.STATE_BYTES for st in states):
            raise ValueError(f"every state is {self.STATE_BYTES} bytes")   # the C side reads n * STATE_BYTES bytes
        c, out = self._merge_draws(draws, len(states), "states")
        _feed.collect(self)
        check(self._lib.h2v_accumulator_merge_states(self._h, b"".join(bytes(st) for st in states), len(states), c, out))
        return self._merged(len(states), out)

    def identify(self):
        """Name the failing proofs of the failing legs: check_legs(), then verify_batch_keys_identify with fresh OS draws over the
        retained inputs of every non-base entry whose pairing fails.  -> {entry: statuses}, statuses[i] what verify_each returns for
        proof i of that leg; for a process_guards leg, guards_check_each over its Guards: 0 or ConstraintSystemFailure per Guard.  Needs
        keep_inputs=True; an add_msm entry that fails is reported with statuses None."""
        if not self._keep_inputs:
            raise ValueError("identify() needs the legs' inputs: create the Accumulator with keep_inputs=True")
        out = {}
        for e, (_, _, ok) in enumerate(self.check_legs()):
            if e == 0 or ok:
                continue
            kept = self._inputs[e]
            if kept is None:
                out[e] = None
                continue
            if kept[0] == "guards":   # a process_guards leg: the verdict of every Guard of its own
                out[e] = [0 if ok_i else PlonkError.ConstraintSystemFailure.value for ok_i in self.ctx.guards_check_each(kept[1])]
                continue
            contexts, keys, proofs, instances = kept
            out[e] = verify_batch_keys_identify(contexts, keys if keys is not None else [0] * len(proofs), proofs, instances)[1]
        return out


class MSMKZG:
    """A device-resident MSMKZG (h2v_msm): the (scalar, base) terms of the reference's MSM trait (poly/commitment.rs:56-79,
    poly/kzg/msm.rs:17-95), kept on the context's GPU in the form the pooled MSM reads in place.  For term lists that live across calls;
    the per-proof feeders (Accumulator.process, process_guards, process_batch) stay the fast paths.  Scalars are ints or 32-byte strings,
    bases 64-byte x | y (all-zero = the identity).  At most 2^24 terms.  A call that raises H2VError leaves the object as it was.
    `context` supplies the device, the params, the stream and the workspaces, and must outlive the object."""

    MAX_TERMS = 1 << 24

    def __init__(self, context: Context):
        if not isinstance(context, Context):
            raise TypeError("MSMKZG takes a Context")
        self.ctx, self._lib = context, context._lib
        self._h = ctypes.c_void_p()
        check(self._lib.h2v_msm_create(context._h, ctypes.byref(self._h)))
        context._adopt(self)

    def _handle(self):
        if not self._h:
            raise ValueError("the MSM object is closed")
        return self._h

    def close(self):
        if self._h:
            self._lib.h2v_msm_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __len__(self):
        n = ctypes.c_size_t(0)
        check(self._lib.h2v_msm_len(self._handle(), ctypes.byref(n)))
        return n.value

    def append_term(self, scalar, base):                       # msm.rs:57-60
        self.append_terms([scalar], [base])

    def append_terms(self, scalars, bases):
        """append_term x n, in order (h2v_msm_append_terms).  A scalar >= r or a base that is not on the curve raises H2VError naming the
        lowest bad term; the object is unchanged."""
        h = self._handle()
        sb, bb, n = _channel((scalars, bases))
        check(self._lib.h2v_msm_append_terms(h, sb, bb, n))

    def add_msm(self, other):                                  # msm.rs:62-65
        """This object's terms, then other's, in order; other is not changed.  other is self raises H2VError."""
        if not isinstance(other, MSMKZG):
            raise TypeError("add_msm takes an MSMKZG")
        check(self._lib.h2v_msm_add_msm(self._handle(), other._handle()))

    def scale(self, factor):                                   # msm.rs:67-75
        """Every scalar times factor mod r, applied at once: scalars() afterwards returns the scaled values."""
        check(self._lib.h2v_msm_scale(self._handle(), _scalar32(factor)))

    def _terms(self, first, count, want_scalars, want_bases):
        h = self._handle()
        n = len(self)
        if count is None:
            count = n - first
        if first < 0 or count < 0 or first + count > n:
            raise ValueError(f"terms [{first}, {first + count}) outside an object of {n}")
        sc = ctypes.create_string_buffer(32 * max(count, 1)) if want_scalars else None
        bs = ctypes.create_string_buffer(64 * max(count, 1)) if want_bases else None
        check(self._lib.h2v_msm_terms(h, first, count, sc, bs))
        return sc, bs, count

    def scalars(self, first=0, count=None):                    # msm.rs:92-94
        """-> the scalars of the terms [first, first + count) as ints"""
        sc, _, k = self._terms(first, count, True, False)
        return [int.from_bytes(sc.raw[32 * i:32 * i + 32], "little") for i in range(k)]

    def bases(self, first=0, count=None):                      # msm.rs:88-90
        """-> the bases of the terms [first, first + count) as 64-byte x | y (zeros = the identity)"""
        _, bs, k = self._terms(first, count, False, True)
        return _points(bs, k)

    def eval(self):                                            # msm.rs:81-86
        """-> 64-byte x | y (zeros = the identity).  One launch for one object: eval_many() takes many."""
        return eval_many([self])[0][0]

    def check(self):                                           # msm.rs:77-79
        return eval_many([self])[1][0]

    def clone(self):
        """A new object with the same terms, independent of this one (create + add_msm)"""
        self._handle()
        m = MSMKZG(self.ctx)
        try:
            m.add_msm(self)
        except Exception:
            m.close()
            raise
        return m


def _handles(msms, what):
    msms = list(msms)
    for m in msms:
        if not isinstance(m, MSMKZG):
            raise TypeError(f"{what} takes MSMKZG objects")
    return msms, (ctypes.c_void_p * max(len(msms), 1))(*[m._handle() for m in msms])


def eval_many(msms):
    """MSMKZG::eval for k objects, one pooled launch per 1024 of them (h2v_msm_eval_many); the same object may occur more than once.
    -> ([64-byte x | y], [is_identity: bool]): the points (zeros = the identity) and MSMKZG::check per object"""
    msms, arr = _handles(msms, "eval_many")
    k = len(msms)
    if not k:
        return [], []
    out = ctypes.create_string_buffer(64 * k)
    ident = (ctypes.c_int * k)()
    check(msms[0]._lib.h2v_msm_eval_many(arr, k, out, ident))
    return _points(out, k), [bool(v) for v in ident]


class DualMSM:
    """Two resident MSMKZG objects and the pairing (poly/kzg/msm.rs:146-204): e(left, s_g2) e(right, -g2) == 1.  Built empty over a
    context, or from two existing objects (which it then owns)."""

    def __init__(self, context: Context, left: MSMKZG = None, right: MSMKZG = None):
        if (left is None) != (right is None):
            raise ValueError("a DualMSM takes both channels or none")
        self.ctx = context
        self.left = left if left is not None else MSMKZG(context)
        try:
            self.right = right if right is not None else MSMKZG(context)
        except Exception:
            self.left.close()
            raise

    def close(self):
        self.left.close()
        self.right.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def scale(self, factor):                                   # msm.rs:173-177
        """Both channels times factor.  The factor is checked before either channel changes."""
        f = _scalar32(factor)
        self.left._handle(), self.right._handle()
        self.left.scale(f)
        self.right.scale(f)

    def add_msm(self, other):                                  # msm.rs:179-183
        """other: a DualMSM, or a Guard as Accumulator.process_guards takes it — ((left_scalars, left_bases), (right_scalars,
        right_bases)) or the dict Context.guard_msm returns — whose terms are appended."""
        if isinstance(other, DualMSM):
            self.left.add_msm(other.left)
            self.right.add_msm(other.right)
            return
        l, r = _guard_sides(other)
        l, r = _channel(l, "left "), _channel(r, "right ")    # (both checked before either channel changes)
        check(self.left._lib.h2v_msm_append_terms(self.left._handle(), *l))
        check(self.right._lib.h2v_msm_append_terms(self.right._handle(), *r))

    def check(self):                                           # msm.rs:185-203
        return dual_check_many([self])[0][0]


def dual_check_many(duals):
    """DualMSM::check for k objects: per 512 of them one pooled MSM over the 2 k channels and one pairing launch
    (h2v_dual_msm_check_many).  -> ([ok: bool], [left_xy], [right_xy]): the raw pairing bit and the evaluated channels per object"""
    duals = list(duals)
    for d in duals:
        if not isinstance(d, DualMSM):
            raise TypeError("dual_check_many takes DualMSM objects")
    k = len(duals)
    if not k:
        return [], [], []
    _, lefts = _handles([d.left for d in duals], "dual_check_many")
    _, rights = _handles([d.right for d in duals], "dual_check_many")
    ok = (ctypes.c_int * k)()
    left, right = ctypes.create_string_buffer(64 * k), ctypes.create_string_buffer(64 * k)
    check(duals[0].left._lib.h2v_dual_msm_check_many(lefts, rights, k, ok, left, right))
    return [bool(v) for v in ok], _points(left, k), _points(right, k)


def _range_args(ranges, names, types):
    """Ranges as tuples of ints, all of one layout -> (k, their columns as arrays of `types`, the result buffers of k range checks)"""
    for r in ranges:   # (uint32 / size_t on the C side: a negative value would wrap around; the library checks the rest)
        if min(r) < 0:
            raise ValueError(f"range {r}: {names} must be non-negative")
    k = len(ranges)
    columns = [(t * max(k, 1))(*[r[j] for r in ranges]) for j, t in enumerate(types)]
    return k, columns, ((ctypes.c_int * max(k, 1))(), ctypes.create_string_buffer(64 * max(k, 1)), ctypes.create_string_buffer(64 * max(k, 1)))


def _range_results(k, ok, left, right):
    """-> (oks, lefts, rights) of k range checks"""
    return [bool(v) for v in ok][:k], _points(left, k), _points(right, k)


def recheck_batches(batches, ranges):
    """Batch.recheck over ranges of several finished batches in one set of launches (h2v_batches_recheck).  batches: Batch objects on
    one device over the same params (keys and shapes may differ); ranges: list of (batch_index, first, count), each inside one group of
    that batch's last finished launch.  -> (oks, lefts, rights): one verdict and the two evaluated channels (64-byte x | y) per range."""
    batches = list(batches)
    if not batches:
        raise ValueError("at least one batch")
    k, columns, out = _range_args([(int(b), int(f), int(c)) for b, f, c in ranges], "the batch index, first and count",
                                  (ctypes.c_uint32, ctypes.c_size_t, ctypes.c_size_t))
    ba = (ctypes.c_void_p * len(batches))(*[b._h.value for b in batches])
    check(batches[0]._lib.h2v_batches_recheck(ba, len(batches), k, *columns, *out))
    return _range_results(k, *out)


def _integer(v, what, kind="an integer", positive=False):
    """v as an int in [0, 2^64), or (0, 2^64) if `positive`; no bool, no float.  kind: what the TypeError says it must be"""
    if isinstance(v, bool) or not isinstance(v, numbers.Integral):
        raise TypeError(f"{what} must be {kind}, got {type(v).__name__}")
    if v < (1 if positive else 0) or v >> 64:
        raise ValueError(f"{what} must be in {'(' if positive else '['}0, 2^64), got {int(v)}")
    return int(v)


def _address(v, what, kind="an integer", positive=False, needed=False):
    """A 16-byte aligned device address as an int, None as 0.  positive: a number given must not be 0; needed: neither None nor 0 will do"""
    v = 0 if v is None else _integer(v, what, kind, positive)
    if needed and not v:
        raise ValueError(f"{what} is missing")
    if v % 16:
        raise ValueError(f"{what} must be 16-byte aligned, got {v:#x}")
    return v


def _check_group_shape(group_sizes, groups, n, nt, draws):
    """What the groups of a batch ask of an upload of n proofs and nt draws (draws: the caller passes some).  Unequal groups (group_sizes):
    their sum, and one draw per proof; equal groups: multiples of their count — groups None leaves that rule to the library."""
    if group_sizes is not None:
        if n != sum(group_sizes):
            raise ValueError(f"the group sizes sum to {sum(group_sizes)} proofs, got {n}")
        if draws and nt != n:
            raise ValueError(f"groups of unequal size take one draw per proof ({n}), got {nt}")
    elif groups is not None and (n % groups or nt % groups):
        raise ValueError(f"n and n_tail must be multiples of the group count ({groups}), got {n} and {nt}")


def _cuda_of(tensor, missing):
    """The cuda namespace (streams, events) of the module a tensor comes from; TypeError(missing) if it has none"""
    cuda = getattr(sys.modules.get(type(tensor).__module__.partition(".")[0]), "cuda", None)
    if cuda is None:
        raise TypeError(missing)
    return cuda


def _device_tensor(t, what, device, dtypes, wanted):
    """What every tensor argument is held to first: a duck-typed tensor, of one of `dtypes` (wanted: the TypeError's words for them), on
    `device` -> (shape, strides)"""
    for attr in ("dtype", "device", "shape", "stride", "data_ptr"):
        if not hasattr(t, attr):
            raise TypeError(f"{what} must be a tensor (no .{attr})")
    if str(t.dtype).rpartition(".")[2] not in dtypes:
        raise TypeError(f"{what} must be {wanted}, got {t.dtype}")
    if getattr(t.device, "type", None) != "cuda" or t.device.index != device:
        raise ValueError(f"{what} must be on the context's device (cuda:{device}), got {t.device}")
    return tuple(t.shape), tuple(t.stride())


class Batch:
    """Staged, device-resident batch (h2v_batch): upload once, launch asynchronously on its stream, finish later.
    Several batches may be in flight on one Context (one HIP stream each)."""

    STAGES = ("decompress", "transcript", "fr_program", "fold", "msm", "pairing", "msm_accumulate")   # the last one lies inside "msm"

    def __init__(self, ctx: Context, max_proofs: int, max_instance_values: int = 0, stream=None, groups: int = 1):
        self.ctx, self._lib = ctx, ctx._lib
        self._h = ctypes.c_void_p()
        check(self._lib.h2v_batch_create(ctx._h, max_proofs, max_instance_values, ctypes.byref(self._h)))
        ctx._adopt(self)
        self.max_proofs = max_proofs
        self.n = 0
        self._keep = None   # upload_tensors: the tensors the enqueued upload reads, until finish()
        self._tails = []    # hold_tail: (event, tensor) of the tensors the library itself made for an upload (a seed's expanded tail)
        self.groups, self.group_sizes = 1, None
        if stream is not None:
            self.set_stream(stream)
        if groups != 1:
            self.set_groups(groups)

    def set_groups(self, groups: int):
        """`groups` independent AccumulatorStrategy batches per upload/launch (h2v_batch_set_groups): group g owns proofs
        [g*n/groups, (g+1)*n/groups) and the same slice of the draws; each has its own accumulators and pairing."""
        check(self._lib.h2v_batch_set_groups(self._h, groups))
        self.groups, self.group_sizes = groups, None

    def set_group_sizes(self, sizes):
        """Groups of unequal size (h2v_batch_set_group_sizes): group g owns the next sizes[g] proofs of later uploads and the same slice
        of the draws, and is exactly verify_batch over them.  1 to 512 sizes, each an integer >= 1, summing to at most max_proofs.  An
        upload then needs sum(sizes) proofs and one draw per proof (or None).  set_groups returns the batch to equal groups."""
        sizes = _group_sizes(sizes)
        if not 1 <= len(sizes) <= MAX_GROUPS:
            raise ValueError(f"a launch holds 1 to {MAX_GROUPS} groups, got {len(sizes)}")
        if sum(sizes) > self.max_proofs:
            raise ValueError(f"the group sizes sum to {sum(sizes)}, above the batch capacity of {self.max_proofs}")
        check(self._lib.h2v_batch_set_group_sizes(self._h, _sizes(sizes), len(sizes)))
        self.groups, self.group_sizes = len(sizes), sizes

    def close(self):
        if self._h:
            self._lib.h2v_batch_destroy(self._h)
            self._h = ctypes.c_void_p()
            self._tails = []   # (the destroy waited for the batch's streams)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def hold_tail(self, tensor):
        """Keep `tensor` — device memory the library itself made for the upload just enqueued, such as a seed's expanded tail, which no
        caller holds — referenced until the batch's stream has passed this point: an event is recorded on the stream now, and the
        tensor is dropped once the event has completed, which the next upload, finish_into() and finish() look at (without waiting).
        So a batch that never waits on the host (upload, launch, finish_into, again) holds the tails of the launches still in
        flight and no more."""
        cuda = _cuda_of(tensor, "the tensor's module has no cuda events to hold it by")
        self._drop_done_tails()
        ev = cuda.Event()
        ev.record(cuda.ExternalStream(self.stream, device=tensor.device))
        self._tails = getattr(self, "_tails", []) + [(ev, tensor)]

    def _drop_done_tails(self, waited=False):
        """Let go of the held tensors whose event has completed (waited: the host has waited for the stream: all of them)"""
        self._tails = [] if waited else [(ev, t) for ev, t in getattr(self, "_tails", []) if not ev.query()]

    def set_stream(self, hip_stream: int):
        self._drop_done_tails()
        check(self._lib.h2v_batch_set_stream(self._h, ctypes.c_void_p(hip_stream)))
        self._drop_done_tails(waited=True)   # (the call waited for the stream it leaves)

    @property
    def stream(self) -> int:
        return self._lib.h2v_batch_stream(self._h) or 0

    def _upload_args(self, proofs_flat, proof_len, instances_flat, col_lens, rand_tail):
        """The arguments h2v_batch_upload and h2v_batch_upload_launch share, n first.  The C side reads n * proof_len,
        n * sum(col_lens) * 32 and n_tail * 32 bytes: the buffers must hold exactly that."""
        n = len(proofs_flat) // proof_len if proof_len else 0
        if proof_len and len(proofs_flat) != n * proof_len:
            raise ValueError("proofs_flat is not a whole number of proofs")
        if len(instances_flat) != n * sum(col_lens) * 32:
            raise ValueError(f"instances_flat must be n * sum(col_lens) * 32 = {n * sum(col_lens) * 32} bytes, got {len(instances_flat)}")
        if rand_tail is not None and len(rand_tail) % 32:
            raise ValueError("rand_tail is not a whole number of 32-byte scalars")
        cl = (ctypes.c_size_t * max(len(col_lens), 1))(*col_lens)
        nt = len(rand_tail) // 32 if rand_tail is not None else 0
        _check_group_shape(getattr(self, "group_sizes", None), None, n, nt, rand_tail is not None)   # (equal groups: the library's H2VError)
        return n, proofs_flat, proof_len, instances_flat, len(col_lens), cl, rand_tail, nt

    def upload(self, proofs_flat: bytes, proof_len: int, instances_flat: bytes, col_lens, rand_tail=None, seed=None, first_index=0, n_tail=None):
        """proofs_flat: n * proof_len bytes; instances_flat: n * sum(col_lens) * 32 bytes;
        rand_tail: bytes of the Fr::random draws of proofs [first, total) of the whole batch (>= n scalars) or None.
        seed (instead of rand_tail): the tail is draws.expand(seed, first_index, n_tail), n_tail = n when None — the draws of a
        32-byte seed (include/h2v_draws.h), expanded on the host."""
        if seed is not None:
            rand_tail = self._seeded_tail(seed, rand_tail, first_index, n_tail, len(proofs_flat) // proof_len if proof_len else 0)[0]
        elif first_index or n_tail is not None:
            raise ValueError("first_index and n_tail go with seed")
        args = self._upload_args(proofs_flat, proof_len, instances_flat, col_lens, rand_tail)
        check(self._lib.h2v_batch_upload(self._h, *args))
        self.n = args[0]

    def upload_device(self, proofs_addr: int, n: int, proof_stride: int, instances_addr, col_lens, rand_addr=None, n_tail=None):
        """upload() for inputs already in device memory (h2v_batch_upload_device), given as addresses: row i of the proofs starts at
        proofs_addr + i * proof_stride (only the VK's proof length of it is read), instances_addr holds n * sum(col_lens) * 32 bytes
        (None when there are none), rand_addr holds n_tail 32-byte draws under upload()'s tail rules — or None: OS draws made on the
        host, the one form that waits for the stream.  Everything is device work on the batch's stream, behind whatever is queued
        there: the caller orders the producers of the inputs before the call and leaves the inputs alone until finish().  A draw >= r
        is found by a kernel and raised by finish() / finish_groups(), which leave the batch empty."""
        n, proof_stride = _integer(n, "n"), _integer(proof_stride, "proof_stride")
        col_lens = [_integer(c, "a column length") for c in col_lens]
        if n > getattr(self, "max_proofs", n):
            raise ValueError(f"n = {n} exceeds the batch capacity of {self.max_proofs}")
        if not proof_stride or proof_stride % 16:
            raise ValueError(f"proof_stride must be a positive multiple of 16, got {proof_stride}")
        proofs_addr = _address(proofs_addr, "proofs_addr", needed=n > 0)
        instances_addr = _address(instances_addr, "instances_addr", needed=n > 0 and sum(col_lens) > 0)
        rand_addr = _address(rand_addr, "rand_addr")
        if not rand_addr:
            if n_tail is not None:
                raise ValueError("n_tail without rand_addr: OS draws are one per proof")
            nt = 0
        else:
            nt = _integer(n if n_tail is None else n_tail, "n_tail")
            if nt < n:
                raise ValueError(f"n_tail = {nt} is below n = {n}")
        _check_group_shape(getattr(self, "group_sizes", None), getattr(self, "groups", 1), n, nt, bool(rand_addr))
        cl = (ctypes.c_size_t * max(len(col_lens), 1))(*col_lens)
        self._keep = None
        self._drop_done_tails()
        check(self._lib.h2v_batch_upload_device(self._h, n, ctypes.c_void_p(proofs_addr), proof_stride, ctypes.c_void_p(instances_addr), len(col_lens), cl,
                                                ctypes.c_void_p(rand_addr), nt))
        self.n = n

    @staticmethod
    def _tensor_bytes(t, what, device, rows=None, row_len=None):
        """A duck-typed tensor as device bytes: uint8, on `device`, 2-D with unit inner stride (`rows` rows; `row_len` given: exactly
        that many bytes per row and no padding between rows) -> (address, rows, row stride)"""
        shape, stride = _device_tensor(t, what, device, ("uint8",), "a uint8 tensor")
        if len(shape) != 2 or (shape[1] > 1 and stride[1] != 1):
            raise ValueError(f"{what} must be 2-D with unit inner stride, got shape {shape} and strides {stride}")
        if rows is not None and shape[0] != rows:
            raise ValueError(f"{what} must hold {rows} rows, got {shape[0]}")
        row_stride = stride[0] if shape[0] > 1 else max(stride[0], shape[1])
        if row_stride < shape[1]:
            raise ValueError(f"{what}: rows overlap (row stride {row_stride} below the row length {shape[1]})")
        if row_len is not None and (shape[1] != row_len or (shape[0] > 1 and row_stride != row_len)):
            raise ValueError(f"{what} must be contiguous rows of {row_len} bytes, got shape {shape} and strides {stride}")
        return int(t.data_ptr()), shape[0], row_stride

    @staticmethod
    def _seeded_tail(seed, rand_tail, first_index, n_tail, n, device=None, stream=None):
        """The tail a seed stands for -> (draws, n_tail): draws.expand(seed, first_index, n_tail) as bytes, or with `device` the same
        as a tensor written by a kernel on `stream` (draws.expand_tensor).  n_tail None: one draw per proof."""
        from . import draws
        if rand_tail is not None:
            raise ValueError("give the draws (rand_tail) or the seed they come from, not both")
        nt = n if n_tail is None else n_tail
        if isinstance(nt, bool) or not isinstance(nt, numbers.Integral) or nt < n:
            raise ValueError(f"n_tail must be an integer >= n = {n}, got {nt!r}")
        if device is None:
            return draws.expand(seed, first_index, nt), nt
        return draws.expand_tensor(seed, first_index, nt, device, stream), nt

    def upload_tensors(self, proofs, instances, col_lens, rand_tail=None, seed=None, first_index=0, n_tail=None):
        """upload_device() from tensors (torch's, or anything with dtype / device / shape / stride() / data_ptr()): proofs [n, >= proof
        length] with any row stride that is a multiple of 16, instances [n, sum(col_lens) * 32] contiguous (None when there are none),
        rand_tail [n_tail, 32] contiguous or None (OS draws).  The batch's stream is made to wait, on the device, for the work queued on
        the tensors' current stream; the tensors are kept referenced until finish().
        seed (instead of rand_tail): the tail is the draws of a 32-byte seed (include/h2v_draws.h), indices [first_index, first_index +
        n_tail) with n_tail = n when None, expanded by a kernel on the batch's stream into a tensor the batch holds until the stream
        has read it (hold_tail) and then taken as rand_tail is: no draw bytes cross to the device, and nothing waits for the stream."""
        if seed is None and (first_index or n_tail is not None):
            raise ValueError("first_index and n_tail go with seed")
        if seed is not None and rand_tail is not None:
            raise ValueError("give the draws (rand_tail) or the seed they come from, not both")
        device = self.ctx.device
        col_lens = list(col_lens)
        addr, n, stride = self._tensor_bytes(proofs, "proofs", device)
        ninst = sum(col_lens) * 32
        iaddr = None
        if ninst:   # (no instance values: `instances` is not looked at)
            if instances is None:
                raise ValueError("instances missing")
            iaddr = self._tensor_bytes(instances, "instances", device, n, ninst)[0]
        raddr = nt = None
        if rand_tail is not None:
            raddr, nt, _ = self._tensor_bytes(rand_tail, "rand_tail", device, None, 32)
        # the inputs are written on the tensors' current stream: the batch's stream waits for it by an event, the host for nothing
        cuda = _cuda_of(proofs, "the tensors' module has no cuda streams to order the upload behind")
        current, mine = cuda.current_stream(proofs.device), self.stream
        if current.cuda_stream != mine:
            ev = cuda.Event()
            ev.record(current)
            cuda.ExternalStream(mine, device=proofs.device).wait_event(ev)
        if seed is not None:   # (behind the wait: the tensor may be memory that work on the current stream still uses)
            rand_tail, nt = self._seeded_tail(seed, None, first_index, n_tail, n, proofs.device, mine)
            raddr = self._tensor_bytes(rand_tail, "rand_tail", device, None, 32)[0]
            if not nt:   # (an upload of no proofs: nothing to draw)
                raddr = nt = None
        try:
            self.upload_device(addr, n, stride, iaddr, col_lens, raddr, nt)
        finally:
            if seed is not None:   # (also when the upload was refused: the expansion is enqueued)
                self.hold_tail(rand_tail)
        self._keep = (proofs, instances, rand_tail)

    def launch(self, with_pairing=True):
        check(self._lib.h2v_batch_launch(self._h, 1 if with_pairing else 0))

    def upload_launch(self, proofs_flat: bytes, proof_len: int, instances_flat: bytes, col_lens, rand_tail=None, with_pairing=True):
        """upload() + launch() with the host -> device copy hidden behind the point decompression (h2v_batch_upload_launch)."""
        args = self._upload_args(proofs_flat, proof_len, instances_flat, col_lens, rand_tail)
        check(self._lib.h2v_batch_upload_launch(self._h, *args, 1 if with_pairing else 0))
        self.n = args[0]

    def export_accumulators(self, device_dst: int):
        check(self._lib.h2v_batch_export_accumulators(self._h, ctypes.c_void_p(device_dst)))

    def fold_check_enqueue(self, device_accumulators: int, n_parts: int):
        check(self._lib.h2v_batch_fold_check_enqueue(self._h, ctypes.c_void_p(device_accumulators), n_parts))

    def finish(self):
        """-> (batch_ok, statuses, left_xy, right_xy)"""
        st = (ctypes.c_int * max(self.n, 1))()
        ok = ctypes.c_int(0)
        left, right = ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
        check(self._lib.h2v_batch_finish(self._h, st, ctypes.byref(ok), left, right))
        self._keep = None   # (upload_tensors' inputs: the enqueued work has run)
        self._drop_done_tails(waited=True)
        return bool(ok.value), memoryview(st).cast('B').cast('i').tolist()[:self.n], left.raw, right.raw

    def finish_groups(self, raw_statuses=False):
        """-> (group_ok[groups], statuses, left_xy[groups], right_xy[groups]).
        `raw_statuses`: the per-proof statuses as the bytes of the C array (n little-endian int32; all zero <=> every proof OK) instead of
        a list — turning 20 480 statuses into Python ints costs 0.15 ms, 5 % of the launch they come from."""
        g = self.groups
        st = (ctypes.c_int * max(self.n, 1))()
        ok = (ctypes.c_int * g)()
        left, right = ctypes.create_string_buffer(64 * g), ctypes.create_string_buffer(64 * g)
        check(self._lib.h2v_batch_finish_groups(self._h, st, ok, left, right, g))
        self._keep = None   # (upload_tensors' inputs: the enqueued work has run)
        self._drop_done_tails(waited=True)
        statuses = bytes(memoryview(st).cast('B')[:4 * self.n]) if raw_statuses else memoryview(st).cast('B').cast('i').tolist()[:self.n]
        return [bool(v) for v in ok], statuses, _points(left, g), _points(right, g)

    SUMMARY_WORDS = 8   # H2V_SUMMARY_WORDS: [draw fault or 0xffffffff, failing proofs, accepted groups, n, groups, flags, 0, 0]

    def finish_device(self, status_addr=None, group_ok_addr=None, left_xy_addr=None, right_xy_addr=None, group_failed_addr=None,
                      failed_index_addr=None, failed_cap=0, summary_addr=None):
        """finish_groups() into device memory (h2v_batch_finish_device), given as addresses, None = not wanted: n int32 statuses, `groups`
        int32 verdicts, 64 bytes per group of either channel, `groups` uint32 counts of failing proofs, the failing proofs' indices in
        ascending order (the first failed_cap of them), SUMMARY_WORDS uint32.  Device work on the batch's stream only: the call waits
        for nothing, leaves the batch's stage alone and may be repeated; the caller orders its readers behind the batch's stream.  The
        batch must be launched (or finished)."""
        addrs = [_address(v, what, "an integer address or None", positive=True)
                 for v, what in ((status_addr, "status_addr"), (group_ok_addr, "group_ok_addr"), (left_xy_addr, "left_xy_addr"),
                                 (right_xy_addr, "right_xy_addr"), (group_failed_addr, "group_failed_addr"),
                                 (failed_index_addr, "failed_index_addr"), (summary_addr, "summary_addr"))]
        failed_cap = _integer(failed_cap, "failed_cap")
        if addrs[5] and not failed_cap:
            raise ValueError("failed_cap must be at least 1 when failed_index_addr is given")
        vp = [ctypes.c_void_p(a) for a in addrs]
        check(self._lib.h2v_batch_finish_device(self._h, *vp[:6], int(failed_cap) if addrs[5] else 0, vp[6]))

    @staticmethod
    def _tensor_words(t, what, device, dtypes, count):
        """A duck-typed tensor as an output array: one of `dtypes`, on `device`, contiguous, `count` elements (None: any number, at
        least one) -> (address, elements)"""
        shape, stride = _device_tensor(t, what, device, dtypes, f"a tensor of {' or '.join(dtypes)}")
        numel, expect = 1, 1
        for size in shape:
            numel *= size
        for size, step in zip(reversed(shape), reversed(stride)):   # (row-major without gaps; a dimension of one element may have any stride)
            if size != 1 and step != expect:
                raise ValueError(f"{what} must be contiguous, got shape {shape} and strides {stride}")
            expect *= size
        if count is None and not numel:
            raise ValueError(f"{what} must hold at least one element")
        if count is not None and numel != count:
            raise ValueError(f"{what} must hold {count} elements, got {numel} (shape {shape})")
        return (int(t.data_ptr()) if numel else None), numel   # (no element: nothing to write, and no address)

    def finish_into(self, status=None, group_ok=None, left_xy=None, right_xy=None, group_failed=None, failed_index=None, summary=None):
        """finish_device() into tensors (torch's, or anything with dtype / device / shape / stride() / data_ptr()), each contiguous and
        on the batch's device, None = not wanted: status int32 [n], group_ok int32 [groups], left_xy / right_xy uint8 [groups, 64],
        group_failed int32 or uint32 [groups], failed_index int32 or uint32 (as many failing proofs as it has elements are reported),
        summary int32 or uint32 [SUMMARY_WORDS].  The batch's stream first waits for the tensors' current stream (whatever made or
        filled them), and that stream then waits, on the device, for the batch's kernels: work queued on it afterwards sees the
        results.  The host waits for nothing; the tensors are the caller's to keep alive until that work has run."""
        device, g = self.ctx.device, self.groups
        words = ("int32", "uint32")
        spec = ((status, "status", ("int32",), self.n), (group_ok, "group_ok", ("int32",), g), (left_xy, "left_xy", ("uint8",), 64 * g),
                (right_xy, "right_xy", ("uint8",), 64 * g), (group_failed, "group_failed", words, g), (failed_index, "failed_index", words, None),
                (summary, "summary", words, self.SUMMARY_WORDS))
        given = [t for t, *_ in spec if t is not None]
        if not given:
            raise ValueError("finish_into: no output tensor given")
        got = [(None, 0) if t is None else self._tensor_words(t, what, device, dtypes, count) for t, what, dtypes, count in spec]
        cuda = _cuda_of(given[0], "the tensors' module has no cuda streams to order the results by")
        current, mine = cuda.current_stream(given[0].device), self.stream
        ordered = current.cuda_stream != mine
        if ordered:
            batch_stream = cuda.ExternalStream(mine, device=given[0].device)
            before = cuda.Event()
            before.record(current)
            batch_stream.wait_event(before)
        self.finish_device(*[a for a, _ in got[:6]], got[5][1], got[6][0])
        if ordered:
            after = cuda.Event()
            after.record(batch_stream)
            current.wait_event(after)
        self._drop_done_tails()

    # ---- every proof's Guard out of the last launch (include/h2v_guards.h; guards.py holds the binding and says what a Guard of a batch is)
    def guard_shape(self):
        """-> (T_L, T_R): the terms of a proof's left and right channel under the plan of the upload"""
        from . import guards
        return guards.guard_shape(self)

    def guards(self, first=0, count=None):
        """The Guards of proofs [first, first + count) (count None: to the end) of the last launch, by one kernel, one copy and one
        synchronise -> one dict per proof as Context.guard_msm returns it (right_scalars, right_bases, left_scalars, left_bases), plus
        mult (32 bytes: the product of the draws behind the proof in its group, which every scalar carries) and status.  The batch
        must be launched or finished; its stage and its results do not change."""
        from . import guards
        return guards.guards(self, first, count)

    def guards_into(self, first=0, count=None, left_scalars=None, left_bases=None, right_scalars=None, right_bases=None, mult=None, status=None):
        """guards() into device memory, tensors or 16-byte aligned device addresses (None = not wanted), by kernels on the batch's
        stream and without a host wait (guards.guards_into)."""
        from . import guards
        return guards.guards_into(self, first, count, left_scalars, left_bases, right_scalars, right_bases, mult, status)

    def guards_append(self, left=None, right=None, first=0, count=None):
        """The range's left terms behind the end of the MSMKZG `left`, its right terms behind the end of `right` (either may be None),
        in the objects' own form -> the number of proofs of the range with a non-zero status (guards.guards_append)."""
        from . import guards
        return guards.guards_append(self, left, right, first, count)

    # ---- point hints (include/h2v_hints.h; hints.py holds the binding and says what a hint is): they change a launch's time, never its results
    def set_hints(self, y32):
        """The claimed y of every point of the current upload, n * n_points * 32 bytes in the proofs' byte order (hints.for_proofs), or
        None to drop them.  The batch must be uploaded and not launched since; every launch of the upload then checks the hints
        instead of taking square roots, and takes the root where a hint does not hold."""
        from . import hints
        return hints.set_hints(self, y32)

    def set_hint_rows(self, rows):
        """set_hints from one row per proof of the current upload — n_points * 32 bytes, or None where the proof's sender gave none
        (include/h2v_hint_rows.h); rows=None drops the hints.  hint_stats() then counts the rows given: n_hinted = n_points * (rows that
        are not None), n_missed = the hints of those rows that were not used."""
        from . import hints
        return hints.set_hint_rows(self, rows)

    def set_hints_tensor(self, t):
        """set_hints from a uint8 tensor [n, 32 * n_points] on the batch's device (row stride a multiple of 16), device -> device on
        the batch's stream, which is made to wait for the tensor's current stream; no host wait."""
        from . import hints
        return hints.set_hints_tensor(self, t)

    def hints(self, first=0, count=None):
        """The canonical y of the points of proofs [first, first + count) of the last launch, count * n_points * 32 bytes (zeros for a
        point that did not decode): hints for the next verifier of the same proofs."""
        from . import hints
        return hints.hints(self, first, count)

    def hints_into(self, t, first=0, count=None):
        """hints() into a uint8 tensor [count, 32 * n_points] on the batch's device (row stride a multiple of 16), by one kernel on the
        batch's stream; the tensor's current stream is made to wait for it, the host for nothing."""
        from . import hints
        return hints.hints_into(self, t, first, count)

    def hint_stats(self):
        """-> (n_points, n_hinted, n_missed) of the last launch: n * n_points; the same if the launch had hints, else 0; the hints not used"""
        from . import hints
        return hints.hint_stats(self)

    def recheck(self, ranges):
        """The pairing checks of ranges of proofs of the last finished launch, on its resident scalars (h2v_batch_recheck).
        ranges: list of (first, count), each inside one group of the launch.  -> (oks, lefts, rights): one verdict and the two
        evaluated channels (64-byte x | y) per range."""
        k, columns, out = _range_args([(int(f), int(c)) for f, c in ranges], "first and count", (ctypes.c_size_t, ctypes.c_size_t))
        check(self._lib.h2v_batch_recheck(self._h, k, *columns, *out))
        return _range_results(k, *out)

    def identify(self, own_records=None):
        """Which proofs of the last finished launch fail the pairing (h2v_batch_identify), whatever closed the launch: its own pairing,
        none, or a later fold.  own_records: the device address (or a tensor) of the records export_accumulators wrote for this launch —
        needed after fold_check_enqueue, which overwrites the batch's own accumulators; None otherwise.
        -> (statuses, group_own_ok[groups], range_checks): statuses[i] is what verify_each returns for proof i, group_own_ok[g] the
        pairing check of group g's own accumulators.  The launch's results are untouched."""
        if own_records is not None and hasattr(own_records, "data_ptr"):
            own_records = own_records.data_ptr()
        st = (ctypes.c_int * max(self.n, 1))()
        own = (ctypes.c_int * self.groups)()
        checks = ctypes.c_size_t(0)
        check(self._lib.h2v_batch_identify(self._h, ctypes.c_void_p(own_records) if own_records is not None else None, st, own, ctypes.byref(checks)))
        return memoryview(st).cast('B').cast('i').tolist()[:self.n], [bool(v) for v in own], checks.value

    PROFILE_KERNEL = 3   # H2V_PROFILE_KERNEL: the dominant kernel's own timestamps only

    def set_profiling(self, on=True):
        """True / 1: an event between the stages and around the dominant kernel (each a barrier packet on the stream);
        Batch.PROFILE_KERNEL: the dominant kernel's own timestamps only (no extra packet); False / 0: off"""
        check(self._lib.h2v_batch_set_profiling(self._h, int(on)))

    def timings_ms(self):
        arr = (ctypes.c_float * len(self.STAGES))()
        k = self._lib.h2v_batch_timings(self._h, arr, len(self.STAGES))
        return dict(zip(self.STAGES, list(arr)[:k]))
