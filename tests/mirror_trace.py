"""What the Python host mirror (halo2_verifier_amd/verifier.py, distributed.py) hands to the C ABI, call by call, recorded through a
stand-in library: no GPU and no real library.  Every scenario below drives public entry points over 2-4 tiny fake proofs; the recorder
notes every h2v_* call with a normalised form of its arguments (integers as they are, size_t / uint32 arrays as lists, byte buffers as
length + SHA-256, proof / instance pointer arrays read with the lengths the same call passes), fills the outputs from a small table
and returns 0.  tests/test_mirror_trace.py compares the result with tests/golden/mirror_calls_python.json, so a change of the mirror
that alters one byte handed to the library, one return value or one refusal shows.

    python tests/mirror_trace.py --write      regenerates the fixture from the mirror as it stands
"""
import ctypes
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import halo2_verifier_amd as h2v   # noqa: E402
from halo2_verifier_amd import _lib, distributed, launch, verifier   # noqa: E402

FIXTURE = os.path.join(HERE, "golden", "mirror_calls_python.json")

# entry points whose proof / instance pointer arrays bring one shape for the call, a shape per proof, or a key per proof:
# name -> (index of `n`, of the proof pointers, of the key indices or None)
_UNIFORM = {"h2v_verify_batch": 1, "h2v_verify_batch_seeded": 1, "h2v_verify_batch_identify": 1, "h2v_verify_batch_seeded_identify": 1, "h2v_verify_each": 1}
_SHAPES = {"h2v_verify_batch_shapes": 1}
_KEYED = {"h2v_verify_batch_keys": (3, 2), "h2v_verify_batch_keys_identify": (3, 2), "h2v_accumulator_process": (4, 3)}

# outputs that are not the default of their type: name -> {argument index: value}
_OUT = {
    "h2v_ctx_proof_shape": {1: 96, 2: 3, 3: 4, 4: 5, 5: 2},
    "h2v_verify_batch_seeded_identify": {16: 0},
    "h2v_accumulator_read": {3: 6, 4: 1},
    "h2v_accumulator_check_legs": {2: 3, 3: [0, 2, 0], 4: [0, 1, 0], 5: [1, 0, 0]},
    "h2v_guard_msm": {8: 2, 11: 1, 13: 3},
}
_RETURNS = {"h2v_batch_stream": 0x7000, "h2v_batch_timings": 7}


def _digest(b):
    return {"len": len(b), "sha256": hashlib.sha256(b).hexdigest()}


def _pointees(arr, lens):
    """the byte strings a pointer array points to, read with the given lengths (never through c_char_p, which stops at a NUL)"""
    addrs = ctypes.cast(arr, ctypes.POINTER(ctypes.c_void_p))
    return [_digest(ctypes.string_at(addrs[i], l)) if addrs[i] else None for i, l in enumerate(lens)]


class Recorder:
    """The stand-in library: every attribute is a callable that records its call, fills the outputs and returns 0"""

    def __init__(self):
        self.calls, self.handles, self.open = [], 0, True

    def __getattr__(self, name):
        if not name.startswith("h2v_"):
            raise AttributeError(name)
        return lambda *args: self._call(name, args)

    def _instance_lens(self, name, args):
        if name in _UNIFORM or name in _SHAPES:
            n, ncols, cl = args[1], args[5], list(args[6])
            if name in _UNIFORM:
                return 2, 4, [32 * sum(cl[:ncols])] * n
            return 2, 4, [32 * sum(cl[i * ncols:(i + 1) * ncols]) for i in range(n)]
        at_n, at_k = _KEYED[name]
        n, keys, ncols, cl = args[at_n], list(args[at_k]), list(args[at_n + 4]), list(args[at_n + 5])
        lens, at = [], 0
        for i in range(n):
            lens.append(32 * sum(cl[at:at + ncols[keys[i]]]))
            at += ncols[keys[i]]
        return at_n + 1, at_n + 3, lens

    def _call(self, name, args):
        pointers = {}
        if name in _UNIFORM or name in _SHAPES or name in _KEYED:
            at_p, at_i, ilens = self._instance_lens(name, args)
            pointers = {at_p: list(args[at_p + 1])[:len(ilens)], at_i: ilens}
        if self.open:
            self.calls.append([name] + [self._norm(a, pointers.get(i)) for i, a in enumerate(args)])
        for i, a in enumerate(args):
            self._fill(a, i, _OUT.get(name, {}).get(i))
        return _RETURNS.get(name, 0)

    def _norm(self, a, lens):
        if a is None or isinstance(a, (bool, int)):
            return a
        if isinstance(a, (bytes, bytearray)):
            return _digest(bytes(a))
        if isinstance(a, ctypes.c_void_p):
            return a.value if a.value is None or a.value < (1 << 32) else "ptr"
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_char_p:
                return {"pointers": len(a), "to": _pointees(a, lens)}
            if a._type_ is ctypes.c_char:
                return {"buffer": len(a)}
            if a._type_ is ctypes.c_int:
                return {"ints_out": len(a)}
            return list(a)
        obj = getattr(a, "_obj", None)   # byref(...)
        if isinstance(obj, ctypes.Structure):
            return {"struct": [getattr(obj, f) for f, _ in obj._fields_]}
        if obj is not None:
            return "out"
        raise TypeError(f"an argument the recorder does not know: {a!r}")

    def _fill(self, a, pos, value):
        if isinstance(a, ctypes.Array):
            if a._type_ is ctypes.c_char:
                a.raw = bytes((pos * 16 + j) & 0xFF for j in range(len(a)))
            elif a._type_ is ctypes.c_int or value is not None:
                for j in range(len(a)):
                    a[j] = value[j] if value is not None and j < len(value) else (-2 if j % 2 and value is None else 0)
            elif a._type_ is ctypes.c_float:
                for j in range(len(a)):
                    a[j] = 0.5 * j
            return
        obj = getattr(a, "_obj", None)
        if isinstance(obj, ctypes.c_void_p):
            self.handles += 1
            obj.value = 0x1000 * self.handles
        elif isinstance(obj, ctypes.c_int):
            obj.value = 1 if value is None else value
        elif isinstance(obj, ctypes.c_size_t):
            obj.value = 3 if value is None else value


class Unreachable:
    def __getattr__(self, name):
        raise AssertionError(f"the C library must not be reached ({name})")


def norm_result(v):
    if isinstance(v, (bytes, bytearray)):
        return _digest(bytes(v))
    if isinstance(v, (list, tuple)):
        return [norm_result(x) for x in v]
    if isinstance(v, dict):
        return {str(k): norm_result(x) for k, x in v.items()}
    if isinstance(v, float):
        return round(v, 6)
    if v is None or isinstance(v, (bool, int, str)):
        return v
    return type(v).__name__


# ---- the fake inputs
def S(v):
    return v.to_bytes(32, "little")


PARAMS = h2v.ParamsKZG((8).to_bytes(4, "little") + bytes(range(160)))
VK_A = h2v.VerifyingKey(b"vk-A\0key", h2v.SerdeFormat.RawBytes)
VK_B = h2v.VerifyingKey(b"vk-B\0key", h2v.SerdeFormat.Processed)
P = [b"proof-%d\0" % i + bytes([i]) * (20 + i) for i in range(4)]              # (a NUL inside: c_char_p indexing would cut it)
U = [[[S(10 * i + 1), S(0)], [S(10 * i + 3)]] for i in range(4)]                # one shape: columns of 2 and 1
M = [[[S(1)], [S(2), 3]], [[4, 5], [S(6)]], [[S(7)], [8, S(9)]], [[], [S(0)]]]   # three shapes, interleaved: a, b, a, c
B64 = [bytes([7 + i]) * 64 for i in range(3)]
SEED = (([1], [B64[0]]), ([S(2), 3], [B64[1], bytearray(B64[2])]))
RAND = [5, S(6), 7, bytearray(S(8))]


def _ctx(vk=VK_A, **kw):
    return h2v.Context(PARAMS, vk, **kw)


def _closing(*objs):
    for o in objs:
        o.close()


def _strategy(items, rand=None, seed=None):
    s = h2v.AccumulatorStrategy(PARAMS, rand=rand) if seed is None else h2v.AccumulatorStrategy.with_accumulator(PARAMS, *seed, rand=rand)
    for vk, inst, proof in items:
        assert h2v.verify_proof(PARAMS, vk, s, inst, proof) is s
    return s


def _finalized(s, identify):
    ok = s.finalize_identify() if identify else s.finalize()
    return [ok] + [getattr(s, k, "unset") for k in ("statuses", "left_xy", "right_xy", "last_range_checks", "last_seed_ok")]


def _batch_pair():
    c = _ctx()
    return c, h2v.Batch(c, 4, 3), h2v.Batch(c, 2, 3, stream=77, groups=2)


FLAT = (b"".join(p[:24] for p in P[:3]), 24, b"".join(S(v) for v in range(9)), [2, 1], b"".join(S(v) for v in (9, 8, 7, 6)))


class _Tensor:
    def data_ptr(self):
        return 0xABC0


def scenarios():
    """name -> callable returning what the Python call returned; everything is created and closed inside"""
    sc = {}

    def one(name):
        def deco(fn):
            sc[name] = fn
            return fn
        return deco

    def with_ctx(name, fn):
        def run():
            c = _ctx()
            try:
                return fn(c)
            finally:
                c.close()
        sc[name] = run

    with_ctx("verify_batch/uniform", lambda c: c.verify_batch(P[:3], U[:3], RAND[:3]))
    with_ctx("verify_batch/mixed_shapes", lambda c: c.verify_batch(P, M, RAND))
    with_ctx("verify_batch/seeded", lambda c: c.verify_batch(P[:2], U[:2], [1, 2], seed=SEED))
    with_ctx("verify_batch/empty", lambda c: c.verify_batch([], [], []))
    with_ctx("verify_batch/empty_seeded", lambda c: c.verify_batch([], [], None, seed=SEED))
    with_ctx("verify_batch/rand_none", lambda c: c.verify_batch(P[:2], U[:2]))
    with_ctx("verify_batch/rand_ints", lambda c: c.verify_batch(P[:2], U[:2], [1 << 255, 2]))
    with_ctx("verify_batch/rand_bytes", lambda c: c.verify_batch([bytearray(P[0]), P[1]], U[:2], [S(3), S(4)]))
    sc["verify_batch/module_function"] = lambda: h2v.verify_batch(PARAMS, VK_A, P[:2], U[:2], [1, 2], device=1)

    def identify(c, **kw):
        r = c.verify_batch_identify(P[:3], U[:3], RAND[:3], **kw)
        return r, c.last_range_checks, c.last_seed_ok
    with_ctx("verify_batch_identify/plain", identify)
    with_ctx("verify_batch_identify/seeded", lambda c: identify(c, seed=SEED))
    with_ctx("verify_batch_identify/empty", lambda c: c.verify_batch_identify([], []))

    with_ctx("verify_each/uniform", lambda c: c.verify_each(P[:3], U[:3]))
    with_ctx("verify_each/three_shapes_interleaved", lambda c: c.verify_each(P, M))
    with_ctx("verify_each/empty", lambda c: c.verify_each([], []))

    def keys(fn, with_unused):
        def run():
            cs = [_ctx(VK_A), _ctx(VK_B)] + ([_ctx(VK_B, device=0)] if with_unused else [])
            try:
                return fn(iter(cs) if with_unused else cs, [1, 0, 1, 0], P, M if with_unused else U, RAND)
            finally:
                _closing(*cs)
        return run
    sc["verify_batch_keys/two_contexts"] = keys(h2v.verify_batch_keys, False)
    sc["verify_batch_keys/context_without_proof"] = keys(h2v.verify_batch_keys, True)
    sc["verify_batch_keys_identify/two_contexts"] = keys(h2v.verify_batch_keys_identify, False)
    sc["verify_batch_keys_identify/context_without_proof"] = keys(h2v.verify_batch_keys_identify, True)
    with_ctx("verify_batch_keys/no_proofs", lambda c: h2v.verify_batch_keys([c], [], [], []))

    one_key = [(VK_A, U[i], P[i]) for i in range(3)]
    same_key_twice = [(h2v.VerifyingKey(VK_A.data, VK_A.format), U[i], P[i]) for i in range(2)]
    two_keys = [(VK_A, U[0], P[0]), (VK_B, U[1], P[1]), (VK_A, U[2], P[2])]
    mixed = [(VK_A, M[i], P[i]) for i in range(4)]
    for ident in (False, True):
        tag = "finalize_identify" if ident else "finalize"
        sc[f"{tag}/empty"] = lambda ident=ident: _finalized(_strategy([]), ident)
        sc[f"{tag}/empty_seeded"] = lambda ident=ident: _finalized(_strategy([], seed=SEED), ident)
        sc[f"{tag}/one_key"] = lambda ident=ident: _finalized(_strategy(one_key, RAND[:3]), ident)
        sc[f"{tag}/one_key_equal_bytes"] = lambda ident=ident: _finalized(_strategy(same_key_twice), ident)
        sc[f"{tag}/one_key_seeded"] = lambda ident=ident: _finalized(_strategy(one_key, RAND[:3], SEED), ident)
        sc[f"{tag}/two_keys"] = lambda ident=ident: _finalized(_strategy(two_keys, RAND[:3]), ident)
        sc[f"{tag}/mixed_shapes"] = lambda ident=ident: _finalized(_strategy(mixed), ident)

    @one("verify_proof/single_strategy")
    def _():
        s = h2v.SingleStrategy(PARAMS, device=2, circuit_instances=2)
        return h2v.verify_proof(PARAMS, VK_A, s, U[0] + U[1], P[0])

    @one("verify_proof/accumulator_strategy")
    def _():
        s = h2v.AccumulatorStrategy(PARAMS, rand=[3], device=1, circuit_instances=2)
        r = h2v.verify_proof(PARAMS, VK_B, s, U[0] + U[1], P[1])
        return r is s, s.finalize(), s.left_xy, s.right_xy

    @one("accumulator/process")
    def _():
        base, ca, cb = h2v.Context(PARAMS), _ctx(VK_A), _ctx(VK_B)
        a = h2v.Accumulator(base)
        out = [a.process(ca, None, P[:2], U[:2], [1, 2]), a.last_all_ok]              # a bare Context, one shape
        out += [a.process(ca, None, P, M), a.process(ca, None, [], [])]               # mixed shapes; no proofs
        out += [a.process([ca, cb], [1, 0, 1], P[:3], U[:3], RAND[:3])]               # a list, one shape
        out += [a.process(iter([ca, cb]), (0, 1, 1, 0), P, M, RAND), a.last_all_ok]   # a list, mixed shapes
        a.add_msm(*SEED)
        out += [a.read(), a.finalize()]
        _closing(a, cb, ca, base)
        return out

    @one("accumulator/journal")
    def _():
        base, ca = h2v.Context(PARAMS), _ctx(VK_A)
        a = h2v.Accumulator(base, journal=8, keep_inputs=True)
        a.process(ca, None, P[:2], M[:2], [1, 2])
        a.add_msm(([], []), SEED[1])
        out = [a.check_legs(), a.identify()]
        a.drop_legs([2])
        a.process([ca], [0, 0], P[2:], U[2:])
        out.append(a.identify())
        a.drop_legs(iter([1]))
        a.drop_legs([])
        a.journal_begin(2)
        a.journal_begin(0)
        out.append(a.check_legs())
        base.close()     # closes the accumulator that lives on it first
        ca.close()
        return out

    @one("batch/upload_launch_finish")
    def _():
        c, b, g = _batch_pair()
        out = [b.stream, b.groups, g.groups]
        b.upload(*FLAT)
        b.launch()
        out.append(b.finish())
        b.upload(FLAT[0], 24, FLAT[2], (2, 1))
        b.launch(with_pairing=False)
        b.export_accumulators(0xD000)
        b.fold_check_enqueue(0xD000, 2)
        out.append(b.finish())
        g.upload_launch(FLAT[0][:48], 24, FLAT[2][:192], [2, 1], FLAT[4], with_pairing=False)
        out.append(g.finish_groups())
        g.upload_launch(FLAT[0][:48], 24, FLAT[2][:192], [2, 1])
        out += [g.finish_groups(raw_statuses=True), g.n]
        g.upload(b"", 0, b"", [0])
        out += [g.finish_groups(), g.n]
        _closing(g, b, c)   # (Context.close() alone would close its batches in the order of a weak set)
        return out

    @one("batch/recheck_identify_misc")
    def _():
        c, b, g = _batch_pair()
        b.upload(*FLAT)
        g.set_groups(1)
        g.set_stream(78)
        g.upload(FLAT[0][:48], 24, FLAT[2][:192], [2, 1])
        out = [b.recheck([(0, 2), (2, 1), (1, 1)]), b.recheck([]), b.recheck(iter([(True, 1.0)]))]
        out += [b.identify(), b.identify(0xE000), g.identify(_Tensor())]
        out += [h2v.recheck_batches([b, g], [(0, 0, 3), (1, 0, 1), (1, 1, 1)]), h2v.recheck_batches(iter([g]), [])]
        b.set_profiling()
        b.set_profiling(h2v.Batch.PROFILE_KERNEL)
        out.append(b.timings_ms())
        _closing(g, b, c)
        return out

    @one("context/other")
    def _():
        c = _ctx(multiopen=h2v.MultiOpen.GWC, transcript=h2v.TranscriptKind.Keccak256, circuit_instances=2, instance_kernel_threshold=9)
        out = [c.msm_g1([1, S(2)], B64[:2]), c.msm_g1([], []), c.pairing_check(B64[0], B64[1]), c.proof_shape()]
        out.append(c.guard_msm(P[0], U[0], cap=4))
        c.set_tuning(frvm_streams=2, msm_window_slots=3)
        c.set_tuning()
        c.close()
        c.close()
        return out

    def batch_factory(c, n, mi, st, g):
        return h2v.Batch(c, n, mi, stream=st, groups=g)

    @one("sharded/local_three_shards_of_two_proofs")
    def _():
        c = _ctx()
        try:
            return distributed.verify_batch_sharded_local(c, P[:2], [U[0], U[0]], [3, 4], 3, batch_factory=batch_factory, device="cpu")
        finally:
            c.close()

    @one("sharded/local_identify")
    def _():
        c = _ctx()
        try:
            return distributed.verify_batch_sharded_local_identify(c, [P[0], P[0], P[0]], [U[1]] * 3, [3, 4, S(5)], 2, batch_factory=batch_factory, device="cpu")
        finally:
            c.close()

    @one("sharded/world_of_one")
    def _():
        c = _ctx()
        try:
            return [distributed.verify_batch_sharded(c, [P[1], P[1]], [U[1]] * 2, [3, 4], batch_factory=batch_factory, device="cpu"),
                    distributed.verify_batch_sharded_identify(c, [], [], [], batch_factory=batch_factory, device="cpu")]
        finally:
            c.close()

    @one("sharded/staged_world_of_one")
    def _():
        c = _ctx()
        sb = distributed.ShardedBatch(c, 3, 3, groups=1, batch_factory=batch_factory, device="cpu")
        sb.upload_launch(*FLAT)
        out = [sb.finish(raw_statuses=True), sb.identify()]
        sb.upload(*FLAT)
        sb.launch()
        out.append(sb.finish())
        sb.close()
        ex = distributed.ShardedBatch(c, 3, 3, batch_factory=batch_factory, device="cpu", always_exchange=True)
        ex.upload_launch(*FLAT)
        out.append(ex.finish())
        ex.upload(*FLAT)
        ex.launch()
        out += [ex.finish(), ex.identify(verdicts=[False])]
        ex.close()
        c.close()
        return out

    return sc


# ---- the refusals: (what raises, the call); the library must not be reached
def refusals():
    def bare(cls, **attrs):
        o = object.__new__(cls)
        o._lib, o._h = Unreachable(), None
        for k, v in attrs.items():
            setattr(o, k, v)
        return o

    c = lambda: bare(h2v.Context)
    acc = lambda **kw: bare(h2v.Accumulator, **kw)
    b = lambda: bare(h2v.Batch)
    p2, u2 = P[:2], U[:2]
    strat = lambda items, rand=None, seed=None: _strategy(items, rand, seed)
    two = [(VK_A, U[0], P[0]), (VK_B, U[1], P[1])]
    sb = lambda: distributed.ShardedBatch(None, 1, batch_factory=lambda *a: b(), device="cpu")
    return {
        "scalar/short_bytes": lambda: c().verify_batch(p2[:1], [[[b"\1" * 31], [S(1)]]], [1]),
        "scalar/int_too_large": lambda: c().verify_batch(p2[:1], [[[1 << 256], [S(1)]]], [1]),
        "scalar/int_negative": lambda: c().msm_g1([-1], B64[:1]),
        "rand/length": lambda: c().verify_batch(p2, u2, [1]),
        "rand/length_identify": lambda: c().verify_batch_identify(p2, u2, [1, 2, 3]),
        "seed/lengths_differ": lambda: c().verify_batch(p2, u2, None, seed=(([1, 2], B64[:1]), ([], []))),
        "seed/base_length": lambda: c().verify_batch(p2, u2, None, seed=(([1], [b"\0" * 63]), ([], []))),
        "seed/not_two_sides": lambda: c().verify_batch_identify(p2, u2, None, seed=(([1], B64[:1]),)),
        "seed/scalar": lambda: c().verify_batch(p2, u2, None, seed=(([b"\1" * 5], B64[:1]), ([], []))),
        "marshal/instance_lists": lambda: c().verify_each(p2, u2[:1]),
        "marshal/proofs_bytes": lambda: c().verify_each(["text"], u2[:1]),
        "marshal/key_index": lambda: h2v.verify_batch_keys([c()], [0, 1], p2, u2),
        "marshal/key_index_negative": lambda: h2v.verify_batch_keys_identify([c(), c()], [0, -1], p2, u2),
        "marshal/column_count": lambda: c().verify_batch(p2, [U[0], U[1][:1]]),
        "tuning/unknown_field": lambda: c().set_tuning(no_such_field=1),
        "tuning/struct_size": lambda: c().set_tuning(struct_size=1),
        "msm_g1/base_length": lambda: c().msm_g1([1], [b"\0" * 63]),
        "msm_g1/lengths_differ": lambda: c().msm_g1([1, 2], B64[:1]),
        "pairing_check/point_length": lambda: c().pairing_check(B64[0], b"\0" * 10),
        "verify_batch/seeded_mixed_shapes": lambda: c().verify_batch(p2, M[:2], None, seed=SEED),
        "verify_batch_identify/mixed_shapes": lambda: c().verify_batch_identify(p2, M[:2]),
        "finalize/rand_length": lambda: strat(two[:1] * 2, rand=[1]).finalize(),
        "finalize_identify/rand_length": lambda: strat(two[:1] * 2, rand=[1, 2, 3]).finalize_identify(),
        "finalize_identify/empty_rand_length": lambda: strat([], rand=[1]).finalize_identify(),
        "finalize/seeded_two_keys": lambda: strat(two, seed=SEED).finalize(),
        "finalize_identify/seeded_two_keys": lambda: strat(two, seed=SEED).finalize_identify(),
        "verify_batch_keys/lengths": lambda: h2v.verify_batch_keys([c()], [0], p2, u2),
        "verify_batch_keys/instance_lengths": lambda: h2v.verify_batch_keys([c()], [0, 0], p2, u2[:1]),
        "verify_batch_keys/no_context": lambda: h2v.verify_batch_keys([], [], [], []),
        "verify_batch_keys_identify/lengths": lambda: h2v.verify_batch_keys_identify([c()], [0, 0, 0], p2, u2),
        "verify_batch_keys_identify/no_context": lambda: h2v.verify_batch_keys_identify(iter(()), [0, 0], p2, u2),
        "verify_batch_keys/bare_context": lambda: h2v.verify_batch_keys(c(), [0, 0], p2, u2),
        "add_msm/lengths_differ": lambda: acc().add_msm(([1], []), ([], [])),
        "add_msm/base_length": lambda: acc().add_msm(([], []), ([1], [b"\0" * 65])),
        "add_msm/base_not_bytes": lambda: acc().add_msm(([1], ["x" * 64]), ([], [])),
        "accumulator/not_a_context": lambda: h2v.Accumulator("ctx"),
        "accumulator/capacity_type": lambda: h2v.Accumulator(c(), journal=2.0),
        "accumulator/capacity_bool": lambda: acc().journal_begin(True),
        "accumulator/capacity_range": lambda: acc().journal_begin(1),
        "accumulator/capacity_max": lambda: h2v.Accumulator(c(), journal=4097),
        "process/context_with_keys": lambda: acc().process(c(), [0, 0], p2, u2),
        "process/list_without_keys": lambda: acc().process([c()], None, p2, u2),
        "process/key_lengths": lambda: acc().process([c()], [0], p2, u2),
        "process/instance_lengths": lambda: acc().process(c(), None, p2, u2[:1]),
        "process/no_context": lambda: acc().process([], [], [], []),
        "process/rand_length": lambda: acc().process(c(), None, p2, u2, [1]),
        "process/key_index": lambda: acc().process([c()], [0, 2], p2, u2),
        "drop_legs/not_integers": lambda: acc().drop_legs([1.0]),
        "drop_legs/bool": lambda: acc().drop_legs([True]),
        "drop_legs/base": lambda: acc().drop_legs([1, 0]),
        "drop_legs/twice": lambda: acc().drop_legs([1, 1]),
        "drop_legs/beyond_the_journal": lambda: acc(_inputs=[None, None]).drop_legs([2]),
        "accumulator/identify_without_inputs": lambda: acc().identify(),
        "recheck_batches/no_batch": lambda: h2v.recheck_batches([], []),
        "recheck_batches/negative": lambda: h2v.recheck_batches([b()], [(0, 1, -1)]),
        "recheck/negative": lambda: b().recheck([(-1, 1)]),
        "upload/whole_proofs": lambda: b().upload(b"\0" * 50, 24, b"", [0]),
        "upload/instances": lambda: b().upload(b"\0" * 48, 24, b"\0" * 32, [1]),
        "upload/rand_tail": lambda: b().upload(b"\0" * 24, 24, b"\0" * 32, [1], b"\0" * 33),
        "upload_launch/whole_proofs": lambda: b().upload_launch(b"\0" * 50, 24, b"", [0]),
        "upload_launch/instances": lambda: b().upload_launch(b"\0" * 48, 24, b"\0" * 32, [1]),
        "upload_launch/rand_tail": lambda: b().upload_launch(b"\0" * 24, 24, b"\0" * 32, [1], b"\0" * 33),
        "distributed/draw_bytes": lambda: distributed.common_draws(1, [b"\1" * 31]),
        "distributed/draw_int": lambda: distributed.common_draws(1, [1 << 256]),
        "distributed/common_draws_length": lambda: distributed.common_draws(2, [1]),
        "distributed/identify_before_finish": lambda: sb().identify(),
        "distributed/instance_lists": lambda: distributed.verify_batch_sharded_local(c(), p2, u2[:1], [1, 2], 1, batch_factory=lambda *a: b(), device="cpu"),
        "distributed/proof_lengths": lambda: distributed.verify_batch_sharded_local(c(), [P[0], P[1]], u2, [1, 2], 1, batch_factory=lambda *a: b(), device="cpu"),
        "distributed/instance_shapes": lambda: distributed.verify_batch_sharded_local(c(), [P[0]] * 2, M[:2], [1, 2], 1, batch_factory=lambda *a: b(), device="cpu"),
        "distributed/zero_draw": lambda: distributed.verify_batch_sharded_local_identify(c(), [P[0]] * 2, u2, [1, 0], 1, batch_factory=lambda *a: b(), device="cpu"),
        "distributed/zero_draw_world": lambda: distributed.verify_batch_sharded_identify(c(), [P[0]] * 2, u2, [S(0), 1], batch_factory=lambda *a: b(), device="cpu"),
        "distributed/local_rand_length": lambda: distributed.verify_batch_sharded_local(c(), p2, u2, [1], 1, batch_factory=lambda *a: b(), device="cpu"),
        "launch/world_size": lambda: launch.spawn_ranks(0, ["true"]),
    }


def record():
    """-> {"scenarios": {name: {"calls": [...], "returned": ...}}, "refusals": {name: [exception type, message]}}"""
    saved = _lib._LIB
    out = {"scenarios": {}, "refusals": {}}
    try:
        for name, fn in scenarios().items():
            rec = _lib._LIB = Recorder()   # Context() and verify_batch_keys* come here through load_library()
            returned = fn()
            rec.open = False
            out["scenarios"][name] = {"calls": json.loads(json.dumps(rec.calls)), "returned": norm_result(returned)}
        _lib._LIB = Unreachable()
        for name, fn in refusals().items():
            try:
                fn()
            except (ValueError, TypeError) as e:
                out["refusals"][name] = [type(e).__name__, str(e)]
            else:
                out["refusals"][name] = ["no exception", ""]
    finally:
        _lib._LIB = saved
    return out


if __name__ == "__main__":
    got = record()
    if "--write" in sys.argv[1:]:
        with open(FIXTURE, "w") as f:
            json.dump(got, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {FIXTURE}: {len(got['scenarios'])} scenarios, {len(got['refusals'])} refusals")
    else:
        with open(FIXTURE) as f:
            want = json.load(f)
        bad = [f"{kind}/{k}" for kind in want for k in set(want[kind]) | set(got[kind]) if want[kind].get(k) != got[kind].get(k)]
        print("\n".join(sorted(bad)) or "the mirror sends what the fixture records")
        sys.exit(1 if bad else 0)
