"""Cost of feeding proofs to a resident accumulator (h2v_accumulator_process x K + h2v_accumulator_finalize) against what the library
offered before it.  Median wall times of --reps runs, host proofs in, one MI355X:
   python tools/accumulator_probe.py [--k 14] [--reps 7] [--out FILE] [--library PATH] [--baseline-only] [--trace]
1. legs:     K = 8 legs of 64 and of 1024 proofs of one key (the k = 14 pool bench.py caches; a leg is the pool's first proofs, every leg
             under draws of its own).  Baseline: the chain of K h2v_verify_batch_seeded calls, each resuming from the (L, R) bytes of the
             one before — the only way to continue an accumulation without the accumulator.
2. one leg:  one process of 1024 proofs of one key against h2v_verify_batch of the same proofs (which runs a pairing; process does not).
3. (--trace) a few process calls only, for a `rocprofv3 --kernel-trace --stats -- python tools/accumulator_probe.py --trace` run that
             gives k_accumulator_scale's own duration.
4. two keys: 2 x 512 interleaved proofs of two k = 8 vector-mul keys in 4 legs against ONE h2v_verify_batch_keys over all 1024.
--library PATH loads another build of libh2v_amd.so; --baseline-only times the baselines alone (a build without the accumulator).
5. (--journal) the leg journal, instead of 1 - 4:
   a. K = 8 legs of 1024 proofs + finalize with the journal on, with it off and (--parent PATH: a libh2v_amd.so built from the parent
      commit, loaded beside the in-tree one) on the parent's library, the variants alternating inside every repetition.
   b. check_legs() and the rebuild drop_legs([]) at 8, 64 and 512 entries (the base and legs of 16 proofs), beside the repair a library without the
      journal offers: a fresh accumulator fed the same legs again from host bytes.
   With --trace: one check_legs and one drop_legs at each of the three sizes, for a `rocprofv3 --kernel-trace --stats` run.
6. (--merge) merging accumulators, instead of 1 - 5; the variants alternate inside every repetition, after >= 50 ms of warm-up:
   a. merge of K = 2, 8, 64 and 512 sources (accumulators fed one leg of 16 proofs) into one destination, against the host round trip a
      caller of the parent commit's library has (--parent PATH): per source read(), then add_msm of the two one-term lists.  merge() runs
      over K distinct accumulators up to 64 (every accumulator owns a stream); merge_states() over K states at every K, the 512 states
      those of 64 accumulators, cycled; the round trip cycles over the same accumulators.
   b. (--parent) process x 8 + finalize on legs of 1024 proofs, this build against the parent's.
   With --trace: at K = 8, 64 and 512, one drop_legs([]) over a journal of K entries (k_fold_records over K whole-point records) and one
   merge_states of K states (k_accumulator_merge_fold over K records), for a `rocprofv3 --kernel-trace --stats` run.
7. (--batch) feeding a finished staged batch, instead of 1 - 6; --parent PATH as above; the variants alternate inside every repetition,
   after >= 50 ms of warm-up:
   a. one RESIDENT launch of 20 x 1024 proofs without a pairing + finish_groups + process_batch, against 20 process calls of 1024 host
      proofs on the parent's library.  Reported, not gated: the two sides differ in where their inputs live.
   b. process_batch alone over a finished batch of G = 20 (x 1024) and G = 512 (x 2) groups, against a merge of G sources on the parent's
      library — the same scale-many + fold shape: h2v_accumulator_merge over 20 accumulators; at 512, where the probe makes no 512
      objects (each owns a stream), h2v_accumulator_merge_states over 512 states.  Gate: process_batch <= 1.25 x the merge.
   With --trace: one process_batch at G = 20 and at G = 512, for a `rocprofv3 --kernel-trace --stats` run."""
import argparse, ctypes, json, os, random, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
bench.hw_queue_env()
from halo2_verifier_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=14)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--library", default=None)
ap.add_argument("--baseline-only", action="store_true")
ap.add_argument("--trace", action="store_true")
ap.add_argument("--journal", action="store_true")
ap.add_argument("--parent", default=None)
ap.add_argument("--merge", action="store_true")
ap.add_argument("--batch", action="store_true")
args = ap.parse_args()
if args.library:
    _lib.lib_path = lambda: os.path.abspath(args.library)
if args.baseline_only:   # a build from before the accumulator exports none of its symbols
    for name in [s for s in _lib.SIGNATURES if s.startswith("h2v_accumulator_")]:
        del _lib.SIGNATURES[name]
import halo2_verifier_amd as h2v

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
RAW = h2v.SerdeFormat.RawBytes
K = 8


def timed(fn):
    fn()   # warm-up: plans, scratch batches, workspaces
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); r = fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], r


n, N = 1024, bench.N_PUBLIC
d = bench.load_or_make_proofs(n, args.k, print)
ctx = h2v.Context(h2v.ParamsKZG(d["params"], RAW), h2v.VerifyingKey(d["vk"], RAW))
P = [d["proofs"][1024 * i:1024 * (i + 1)] for i in range(n)]
I = [[[d["inst"][32 * (N * i + j):32 * (N * i + j + 1)] for j in range(N)]] for i in range(n)]
rnd = random.Random(2025)
draws = [[rnd.randrange(1, R_MOD) for _ in range(n)] for _ in range(K)]


def seeded_chain(m):
    """K legs of the pool's first m proofs through h2v_verify_batch_seeded, each from the bytes of the one before"""
    L = R = None
    ok = True
    for j in range(K):
        seed = (([], []), ([], [])) if L is None else (([1], [L]), ([1], [R]))
        okj, _, L, R = ctx.verify_batch(P[:m], I[:m], draws[j][:m], seed=seed)
        ok = ok and okj
    return ok, L, R


def accumulator_legs(m):
    acc = h2v.Accumulator(ctx)
    for j in range(K):
        acc.process(ctx, None, P[:m], I[:m], draws[j][:m])
    r = acc.finalize()
    acc.close()
    return r


res = {"k": args.k, "reps": args.reps, "legs": K, "library": args.library or "in-tree", "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES")}


def median(ts):
    return sorted(ts)[len(ts) // 2]


def parent_context(path):
    """a Context on another build of the library, loaded beside the in-tree one (a parent build lacks the journal's symbols)"""
    lib = ctypes.CDLL(os.path.abspath(path))
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    mine = _lib.load_library()
    _lib._LIB = lib
    try:
        return h2v.Context(h2v.ParamsKZG(d["params"], RAW), h2v.VerifyingKey(d["vk"], RAW))
    finally:
        _lib._LIB = mine


def journal_probe():
    LEG, SIZES = 16, (8, 64, 512)

    def journaled(J):
        """a journal of J entries: the (empty) base and J - 1 legs"""
        acc = h2v.Accumulator(ctx, journal=J)
        for j in range(J - 1):
            acc.process(ctx, None, P[:LEG], I[:LEG], draws[j % K][:LEG])
        return acc

    if args.trace:
        for J in SIZES:
            acc = journaled(J)
            before = acc.read()
            assert all(ok for _, _, ok in acc.check_legs())
            acc.drop_legs([])
            assert acc.read() == before
            acc.close()
        return
    # a. 8 legs of 1024 + finalize
    variants = {"journal_on": (ctx, K + 1), "journal_off": (ctx, 0)}
    if args.parent:
        variants["parent"] = (parent_context(args.parent), 0)

    def legs(c, journal):
        acc = h2v.Accumulator(c, journal=journal) if journal else h2v.Accumulator(c)
        for j in range(K):
            acc.process(c, None, P, I, draws[j])
        r = acc.finalize()
        acc.close()
        return r
    want = legs(ctx, 0)
    assert want[0]
    ts = {v: [] for v in variants}
    for v, (c, journal) in variants.items():
        assert legs(c, journal) == want   # warm-up
    for _ in range(args.reps):
        for v, (c, journal) in variants.items():
            t0 = time.perf_counter(); legs(c, journal); ts[v].append((time.perf_counter() - t0) * 1e3)
    row = {v: round(median(t), 3) for v, t in ts.items()}
    row.update({v + "_min_max": [round(min(t), 3), round(max(t), 3)] for v, t in ts.items()})
    line = f"{K} legs of 1024 + finalize: " + "   ".join(f"{v} {row[v]:.3f} ms" for v in variants)
    if args.parent:
        for v in ("journal_on", "journal_off"):
            row[v + "_over_parent"] = round(row[v] / row["parent"], 4)
            line += f"   {v} / parent {row[v + '_over_parent']:.3f}x ({'within' if row[v + '_over_parent'] <= 1.08 else 'OUTSIDE'} 1.08x)"
    res["legs_1024_ms"] = row
    print(line, flush=True)
    # b. check_legs and the rebuild at 8, 64, 512 entries of 16 proofs; the repair without the journal beside them
    res["journal_ops_ms"] = {}
    for J in SIZES:
        acc = journaled(J)
        before = acc.read()
        t_check, got = timed(acc.check_legs)
        assert len(got) == J and all(ok for _, _, ok in got)
        t_drop, _ = timed(lambda: acc.drop_legs([]))
        assert acc.read() == before
        acc.close()

        def refeed():
            fresh = h2v.Accumulator(ctx)
            for j in range(J - 1):
                fresh.process(ctx, None, P[:LEG], I[:LEG], draws[j % K][:LEG])
            r = fresh.read()
            fresh.close()
            return r
        t_feed, again = timed(refeed)
        assert again == before
        res["journal_ops_ms"][J] = {"check_legs_ms": round(t_check, 3), "drop_legs_ms": round(t_drop, 3), "refeed_ms": round(t_feed, 3)}
        print(f"{J:4d} entries, legs of {LEG}: check_legs {t_check:8.3f} ms   drop_legs (rebuild) {t_drop:8.3f} ms   a fresh accumulator fed again {t_feed:9.3f} ms", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def merge_probe():
    LEG, SIZES, OBJECTS = 16, (2, 8, 64, 512), 64

    def fed(c, j):
        acc = h2v.Accumulator(c)
        acc.process(c, None, P[:LEG], I[:LEG], draws[j % K][j % 7:j % 7 + LEG])
        return acc

    cs = [rnd.randrange(1, R_MOD) for _ in range(max(SIZES))]
    if args.trace:
        srcs = [fed(ctx, j) for j in range(8)]
        states = [a.export_state() for a in srcs]
        for J in (8, 64, 512):
            acc = h2v.Accumulator(ctx, journal=J)
            acc.merge_states([states[k % 8] for k in range(J - 1)], cs[:J - 1])      # a journal of J entries, the base included
            before = acc.read()
            acc.drop_legs([])                                                       # k_fold_records over J records
            assert acc.read() == before
            acc.close()
            acc = h2v.Accumulator(ctx)
            acc.merge_states([states[k % 8] for k in range(J)], cs[:J])             # k_accumulator_merge_fold over J records
            acc.close()
        for a in srcs:
            a.close()
        return
    srcs = [fed(ctx, j) for j in range(OBJECTS)]
    states = [a.export_state() for a in srcs]
    pctx = parent_context(args.parent) if args.parent else None
    psrcs = [fed(pctx, j) for j in range(OBJECTS)] if pctx else []
    assert not psrcs or [a.read() for a in psrcs] == [a.read() for a in srcs]
    res["merge_ms"] = {}
    for Kn in SIZES:
        variants = {}
        dst = h2v.Accumulator(ctx)
        if Kn <= OBJECTS:
            variants["merge"] = lambda: dst.merge(srcs[:Kn], cs[:Kn])
        variants["merge_states"] = lambda: dst.merge_states([states[k % OBJECTS] for k in range(Kn)], cs[:Kn])
        if pctx:
            pdst = h2v.Accumulator(pctx)

            def round_trip():
                for k in range(Kn):
                    left, right, _, _ = psrcs[k % OBJECTS].read()
                    pdst.add_msm(([cs[k]], [left]), ([cs[k]], [right]))
            variants["parent_round_trip"] = round_trip
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.05:   # warm-up
            for fn in variants.values():
                fn()
        ts = {v: [] for v in variants}
        for _ in range(args.reps):
            for v, fn in variants.items():
                t0 = time.perf_counter(); fn(); ts[v].append((time.perf_counter() - t0) * 1e3)
        row = {v: round(median(t), 3) for v, t in ts.items()}
        row.update({v + "_min_max": [round(min(t), 3), round(max(t), 3)] for v, t in ts.items()})
        res["merge_ms"][Kn] = row
        print(f"{Kn:4d} sources of {LEG} proofs: " + "   ".join(f"{v} {row[v]:9.3f} ms" for v in variants), flush=True)
        dst.close()
        if pctx:
            pdst.close()
    for a in srcs + psrcs:
        a.close()
    if pctx:
        def legs(c):
            acc = h2v.Accumulator(c)
            for j in range(K):
                acc.process(c, None, P, I, draws[j])
            r = acc.finalize()
            acc.close()
            return r
        variants = {"this_build": ctx, "parent": pctx}
        want = legs(ctx)
        assert want[0] and legs(pctx) == want   # warm-up
        ts = {v: [] for v in variants}
        for _ in range(args.reps):
            for v, c in variants.items():
                t0 = time.perf_counter(); legs(c); ts[v].append((time.perf_counter() - t0) * 1e3)
        row = {v: round(median(t), 3) for v, t in ts.items()}
        row.update({v + "_min_max": [round(min(t), 3), round(max(t), 3)] for v, t in ts.items()})
        row["this_over_parent"] = round(row["this_build"] / row["parent"], 4)
        res["legs_1024_ms"] = row
        print(f"{K} legs of 1024 + finalize: this build {row['this_build']:.3f} ms   parent {row['parent']:.3f} ms   ratio {row['this_over_parent']:.3f}x "
              f"({'within' if row['this_over_parent'] <= 1.08 else 'OUTSIDE'} 1.08x)", flush=True)
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


def batch_probe():
    LEGS = 20
    flat_p, flat_i = d["proofs"][:1024 * n], d["inst"][:32 * N * n]

    def staged(groups, per_group):
        """a resident batch of groups x per_group proofs (the pool, cycled), uploaded once"""
        total = groups * per_group
        reps_, rest = divmod(total, n)
        b = h2v.Batch(ctx, total, N, groups=groups)
        tail = b"".join(rnd.randrange(1, R_MOD).to_bytes(32, "little") for _ in range(total))
        b.upload(flat_p * reps_ + flat_p[:1024 * rest], 1024, flat_i * reps_ + flat_i[:32 * N * rest], [N], tail)
        return b

    big, wide = staged(LEGS, n), staged(512, 2)
    for b in (big, wide):
        b.launch(with_pairing=False)
        ok, st, _, _ = b.finish_groups(raw_statuses=True)
        assert all(ok) and not any(st)
    if args.trace:
        for b in (big, wide):
            acc = h2v.Accumulator(ctx)
            acc.process(ctx, None, P[:8], I[:8], draws[1][:8])
            assert acc.process_batch(b) == (b.n, 0) and acc.finalize()[0]
            acc.close()
        return
    pctx = parent_context(args.parent) if args.parent else None
    res["batch_ms"] = {}

    def alternate(variants):
        t0 = time.perf_counter()
        while time.perf_counter() - t0 < 0.05:   # warm-up
            for fn in variants.values():
                fn()
        ts = {v: [] for v in variants}
        for _ in range(args.reps):
            for v, fn in variants.items():
                t0 = time.perf_counter(); fn(); ts[v].append((time.perf_counter() - t0) * 1e3)
        row = {v: round(median(t), 3) for v, t in ts.items()}
        row.update({v + "_min_max": [round(min(t), 3), round(max(t), 3)] for v, t in ts.items()})
        return row

    # a. launch + finish_groups + process_batch of 20 x 1024 resident proofs, against 20 process calls of 1024 host proofs
    acc = h2v.Accumulator(ctx)

    def resident():
        big.launch(with_pairing=False)
        big.finish_groups(raw_statuses=True)
        return acc.process_batch(big)
    variants = {"launch_finish_process_batch": resident}
    if pctx:
        pacc = h2v.Accumulator(pctx)

        def host_legs():
            for j in range(LEGS):
                pacc.process(pctx, None, P, I, draws[j % K])
        variants["parent_process_x20"] = host_legs
    row = alternate(variants)
    assert acc.finalize()[0]
    line = f"{LEGS} x 1024 proofs: " + "   ".join(f"{v} {row[v]:9.3f} ms" for v in variants)
    if pctx:
        row["parent_over_this"] = round(row["parent_process_x20"] / row["launch_finish_process_batch"], 2)
        line += f"   ({row['parent_over_this']:.1f}x; resident inputs against host bytes: reported, not gated)"
        pacc.close()
    res["batch_ms"]["resident_20x1024"] = row
    print(line, flush=True)
    acc.close()
    # b. process_batch alone, against a merge of as many sources on the parent's library
    cs = [rnd.randrange(1, R_MOD) for _ in range(512)]
    for b, G in ((big, LEGS), (wide, 512)):
        acc = h2v.Accumulator(ctx)
        acc.process(ctx, None, P[:8], I[:8], draws[1][:8])   # (a non-empty accumulator: the scale step has points to scale)
        variants = {"process_batch": lambda: acc.process_batch(b)}
        psrcs = []
        if pctx:
            pdst = h2v.Accumulator(pctx)
            for j in range(min(G, LEGS)):
                a = h2v.Accumulator(pctx)
                a.process(pctx, None, P[:16], I[:16], draws[j % K][:16])
                psrcs.append(a)
            if G <= LEGS:
                variants["parent_merge"] = lambda: pdst.merge(psrcs, cs[:G])
            else:
                states = [a.export_state() for a in psrcs]
                variants["parent_merge_states"] = lambda: pdst.merge_states([states[k % len(states)] for k in range(G)], cs[:G])
        row = alternate(variants)
        line = f"G = {G:3d}: " + "   ".join(f"{v} {row[v]:8.3f} ms" for v in variants)
        if pctx:
            other = [v for v in variants if v != "process_batch"][0]
            row["over_merge"] = round(row["process_batch"] / row[other], 4)
            line += f"   ratio {row['over_merge']:.3f}x ({'within' if row['over_merge'] <= 1.25 else 'OUTSIDE'} 1.25x)"
            pdst.close()
        res["batch_ms"][f"process_batch_G{G}"] = row
        print(line, flush=True)
        assert acc.finalize()[0]
        acc.close()
        for a in psrcs:
            a.close()
    big.close(); wide.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)


if args.batch:
    batch_probe()
    ctx.close()
    sys.exit(0)
if args.merge:
    merge_probe()
    ctx.close()
    sys.exit(0)
if args.journal:
    journal_probe()
    ctx.close()
    sys.exit(0)
if args.trace:
    acc = h2v.Accumulator(ctx)
    for j in range(K):
        acc.process(ctx, None, P, I, draws[j])
    assert acc.finalize()[0]
    acc.close()
    ctx.close()
    sys.exit(0)

res["legs_ms"] = {}
for m in (64, 1024):
    t0, want = timed(lambda: seeded_chain(m))
    assert want[0]
    row = {"seeded_chain_ms": round(t0, 3)}
    line = f"{K} legs of {m:4d}: seeded chain {t0:9.3f} ms"
    if not args.baseline_only:
        t1, got = timed(lambda: accumulator_legs(m))
        assert got == want, "the accumulator's legs and the seeded chain disagree"
        row["accumulator_ms"] = round(t1, 3)
        line += f"   process x {K} + finalize {t1:9.3f} ms   ({t1 / t0:.3f}x)"
    res["legs_ms"][m] = row
    print(line, flush=True)

t0, r = timed(lambda: ctx.verify_batch(P, I, draws[0]))
assert r[0]
res["one_leg_ms"] = {"verify_batch_ms": round(t0, 3)}
line = f"one leg of 1024: verify_batch {t0:9.3f} ms"
if not args.baseline_only:
    acc = h2v.Accumulator(ctx)
    acc.process(ctx, None, P[:8], I[:8], draws[1][:8])   # (a non-empty accumulator: the scale step has points to scale)
    t1, st = timed(lambda: acc.process(ctx, None, P, I, draws[0]))
    assert st == [0] * n and acc.finalize()[0]
    acc.close()
    res["one_leg_ms"]["process_ms"] = round(t1, 3)
    line += f"   process {t1:9.3f} ms   ({t1 / t0:.3f}x)"
print(line, flush=True)
ctx.close()

# two keys at k = 8 (the bench pool has one key)
import circuits
POOL = 64
setups = [circuits.setup_vector_mul(8, m) for m in (8, 7)]
pools = [circuits.prove_vector_mul_batch(s, POOL, seed=100 + k, threads=16) for k, s in enumerate(setups)]
ctxs = [h2v.Context(h2v.ParamsKZG(s.params, RAW), h2v.VerifyingKey(s.vk, RAW)) for s in setups]
keys = [i % 2 for i in range(n)]
P2 = [pools[k][0][(i // 2) % POOL] for i, k in enumerate(keys)]
I2 = [pools[k][1][(i // 2) % POOL] for i, k in enumerate(keys)]
t0, want = timed(lambda: h2v.verify_batch_keys(ctxs, keys, P2, I2, draws[0]))
assert want[0]
res["two_keys_ms"] = {"verify_batch_keys_ms": round(t0, 3)}
line = f"two keys, 1024:  verify_batch_keys {t0:9.3f} ms"
if not args.baseline_only:
    def four_legs():
        acc = h2v.Accumulator(ctxs[0])
        st = []
        for a in range(0, n, n // 4):
            st += acc.process(ctxs, keys[a:a + n // 4], P2[a:a + n // 4], I2[a:a + n // 4], draws[0][a:a + n // 4])
        ok, left, right = acc.finalize()
        acc.close()
        return ok, st, left, right
    t1, got = timed(four_legs)
    assert got == want
    res["two_keys_ms"]["four_legs_ms"] = round(t1, 3)
    line += f"   4 legs of 256 + finalize {t1:9.3f} ms   ({t1 / t0:.3f}x)"
print(line, flush=True)
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
for c in ctxs:
    c.close()
for s in setups:
    s.free()
