"""Cost of finding the proofs that made a batch fail (h2v_verify_batch_identify) on ONE batch of 1024 proofs, against the batch alone
(h2v_verify_batch) and against SingleStrategy for every proof (h2v_verify_each); plus the cost of one round of re-checks by its width
(h2v_batch_recheck on a staged batch).  Median wall times of --reps runs, resident inputs:
   python tools/identify_probe.py [--k 14] [--reps 7] [--out FILE]
The proofs are the k = 14 pool bench.py caches (made here, from the same seeds, if no cache holds it).  A bad proof is a good one with
the sign of h2 flipped: it decodes and passes the transcript, only the pairing rejects it.
   python tools/identify_probe.py --keys 1,2,4,8 [--reps 7] [--out FILE]
measures identification over several VerifyingKeys instead (h2v_verify_batch_keys_identify): V distinct k = 8 vector-mul VKs over one
setup, 1024 proofs interleaved (proof i belongs to key i mod V), 0 / 1 / 4 / 32 / all bad, next to h2v_verify_batch_keys and to
h2v_verify_each summed over the keys; the pass path with two instance shapes per key; and one pooled round of re-checks over V staged
batches (h2v_batches_recheck) against the same ranges re-checked batch by batch.
   python tools/identify_probe.py --parent PATH [--k 14] [--reps 7] [--out FILE]
compares this build with another build of libh2v_amd.so (PATH: one made from the parent commit, loaded beside the in-tree one): one
round of re-checks of 1 range of 1024, 8 of 128, 32 of 32 and 32 single proofs, and the 0-bad pass path of h2v_verify_batch_identify,
the two builds alternating inside every repetition; medians, and each build's min - max spread."""
import argparse, ctypes, json, os, random, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
bench.hw_queue_env()
import halo2_verifier_amd as h2v

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=14)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--keys", default=None, help="comma-separated key counts: identification over several VerifyingKeys")
ap.add_argument("--parent", default=None, help="another build of libh2v_amd.so to compare the re-check rounds with")
args = ap.parse_args()


def timed(fn):
    fn()   # warm-up: plans, scratch batch, workspaces
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); r = fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], r


def flip_h2(p):
    b = bytearray(p); b[-1] ^= 0x40
    return bytes(b)


def several_keys(counts):
    import circuits
    n, pool = 1024, 64
    n_mul = [8, 7, 6, 5, 4, 3, 9, 10]
    raw = h2v.SerdeFormat.RawBytes
    setups = [circuits.setup_vector_mul(8, m) for m in n_mul[:max(counts)]]
    pools = [circuits.prove_vector_mul_batch(s, pool, seed=100 + k, threads=16) for k, s in enumerate(setups)]
    ctxs = [h2v.Context(h2v.ParamsKZG(s.params, raw), h2v.VerifyingKey(s.vk, raw)) for s in setups]
    rnd = random.Random(2026)
    rand = [rnd.randrange(1, R_MOD) for _ in range(n)]
    res = {"n": n, "k": 8, "reps": args.reps, "keys": {}}
    for V in counts:
        keys = [i % V for i in range(n)]
        P = [pools[k][0][(i // V) % pool] for i, k in enumerate(keys)]
        I = [pools[k][1][(i // V) % pool] for i, k in enumerate(keys)]
        cs = ctxs[:V]
        r = res["keys"][V] = {}
        t, out = timed(lambda: h2v.verify_batch_keys(cs, keys, P, I, rand))
        assert out[0]
        r["verify_batch_keys_ms"] = round(t, 3)
        print(f"V={V}: verify_batch_keys, 1024 good:        {t:8.3f} ms", flush=True)
        for nb in (0, 1, 4, 32, n):
            bad = sorted(rnd.sample(range(n), nb))
            Q = list(P)
            for i in bad:
                Q[i] = flip_h2(Q[i])
            t, out = timed(lambda: h2v.verify_batch_keys_identify(cs, keys, Q, I, rand))
            assert [i for i in range(n) if out[1][i]] == bad and all(out[1][i] == -2 for i in bad)
            r[f"identify_{nb}_bad"] = {"ms": round(t, 3), "range_checks": out[4]}
            print(f"V={V}: verify_batch_keys_identify, {nb:4d} bad: {t:8.3f} ms   {out[4]:4d} range checks", flush=True)
            if nb == 4:
                def each():
                    for k in range(V):
                        idx = [i for i in range(n) if keys[i] == k]
                        cs[k].verify_each([Q[i] for i in idx], [I[i] for i in idx])
                t, _ = timed(each)
                r["verify_each_sum_ms"] = round(t, 3)
                print(f"V={V}: verify_each over every key:        {t:8.3f} ms", flush=True)
        # the pass path with two instance shapes per key: every other proof of a key has its last product not public
        alt = [circuits.prove_vector_mul_len(setups[k], [1] * setups[k].n_mul, [1] * (setups[k].n_mul - 1) + [0], setups[k].n_mul - 1, rng_seed=k)
               for k in range(V)]
        P2 = [p if (i // V) % 2 == 0 else alt[keys[i]][0] for i, p in enumerate(P)]
        I2 = [inst if (i // V) % 2 == 0 else alt[keys[i]][1] for i, inst in enumerate(I)]
        t, out = timed(lambda: h2v.verify_batch_keys(cs, keys, P2, I2, rand))
        assert out[0]
        t2, out2 = timed(lambda: h2v.verify_batch_keys_identify(cs, keys, P2, I2, rand))
        assert out2[0] and out2[4] == 0
        r["two_shapes"] = {"verify_batch_keys_ms": round(t, 3), "identify_ms": round(t2, 3)}
        print(f"V={V}: two shapes per key: verify_batch_keys {t:8.3f} ms, identify (pass) {t2:8.3f} ms", flush=True)
        # one round over V staged batches (one per key, n / V proofs each), pooled against the same ranges batch by batch
        bs = []
        for k in range(V):
            idx = [i for i in range(n) if keys[i] == k]
            b = h2v.Batch(cs[k], len(idx), 8)
            b.upload(b"".join(P[i] for i in idx), len(P[0]), b"".join(b"".join(I[i][0]) for i in idx), [len(I[idx[0]][0])],
                     b"".join(rand[i].to_bytes(32, "little") for i in idx))
            b.launch(); b.finish()
            bs.append(b)
        for per, size in ((32, n // V // 32), (32, 1), (128, 1)):
            ranges = [(k, j * (n // V // per), size) for k in range(V) for j in range(per)]
            t, out = timed(lambda: h2v.recheck_batches(bs, ranges))
            assert all(out[0])
            t1, _ = timed(lambda: [bs[k].recheck([(f, c) for kk, f, c in ranges if kk == k]) for k in range(V)])
            r[f"round_{per}x{size}_per_batch"] = {"pooled_ms": round(t, 3), "batch_by_batch_ms": round(t1, 3)}
            print(f"V={V}: a round of {V}x{per} ranges of {size:3d}: pooled {t:8.3f} ms, batch by batch {t1:8.3f} ms", flush=True)
        for b in bs:
            b.close()
    for c in ctxs:
        c.close()
    for s in setups:
        s.free()
    return res


if args.keys:
    res = several_keys([int(v) for v in args.keys.split(",")])
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    sys.exit(0)

n, N = 1024, bench.N_PUBLIC
d = bench.load_or_make_proofs(n, args.k, print)
ctx = h2v.Context(h2v.ParamsKZG(d["params"], h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(d["vk"], h2v.SerdeFormat.RawBytes))
P = [d["proofs"][1024 * i:1024 * (i + 1)] for i in range(n)]
I = [[[d["inst"][32 * (N * i + j):32 * (N * i + j + 1)] for j in range(N)]] for i in range(n)]
rnd = random.Random(2024)
rand = [rnd.randrange(1, R_MOD) for _ in range(n)]


def spoiled(bad):
    Q = list(P)
    for i in bad:
        b = bytearray(Q[i]); b[-1] ^= 0x40; Q[i] = bytes(b)
    return Q




def against_parent(path):
    from halo2_verifier_amd import _lib
    lib = ctypes.CDLL(os.path.abspath(path))   # (a parent build lacks the newer symbols)
    for name, (restype, argtypes) in _lib.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = restype, argtypes
    mine = _lib.load_library()
    _lib._LIB = lib
    try:
        pctx = h2v.Context(h2v.ParamsKZG(d["params"], h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(d["vk"], h2v.SerdeFormat.RawBytes))
    finally:
        _lib._LIB = mine
    builds = {"this": ctx, "parent": pctx}
    staged = {}
    for v, c in builds.items():
        b = h2v.Batch(c, n, N)
        b.upload(d["proofs"], 1024, d["inst"], [N], b"".join(x.to_bytes(32, "little") for x in rand))
        b.launch(); b.finish()
        staged[v] = b
    res = {"n": n, "k": args.k, "reps": args.reps, "parent": path, "rows": {}}

    def alternate(name, fns):
        """fns: build -> a call; warm-up, then args.reps repetitions with the builds alternating inside each"""
        want = None
        for v, fn in fns.items():
            got = fn()
            assert want is None or got == want, name   # both builds give the same answer
            want = got
        ts = {v: [] for v in fns}
        for _ in range(args.reps):
            for v, fn in fns.items():
                t0 = time.perf_counter(); fn(); ts[v].append((time.perf_counter() - t0) * 1e3)
        row = {}
        for v, t in ts.items():
            row[v] = {"median_ms": round(sorted(t)[len(t) // 2], 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3)}
        spread = row["parent"]["max_ms"] - row["parent"]["min_ms"]
        row["parent_spread_ms"] = round(spread, 3)
        row["this_minus_parent_ms"] = round(row["this"]["median_ms"] - row["parent"]["median_ms"], 3)
        res["rows"][name] = row
        print(f"{name:28s} this {row['this']['median_ms']:7.3f} ms [{row['this']['min_ms']:.3f} .. {row['this']['max_ms']:.3f}]   "
              f"parent {row['parent']['median_ms']:7.3f} ms [{row['parent']['min_ms']:.3f} .. {row['parent']['max_ms']:.3f}]   "
              f"difference {row['this_minus_parent_ms']:+.3f} ms, parent's spread {spread:.3f} ms", flush=True)

    for width, size in ((1, 1024), (8, 128), (32, 32), (32, 1)):
        ranges = [(i * (n // width), size) for i in range(width)] if size > 1 else [(i, 1) for i in range(width)]
        alternate(f"recheck {width} x {size}", {v: (lambda b=b: b.recheck(ranges)[0]) for v, b in staged.items()})
    alternate("verify_batch_identify, 0 bad", {v: (lambda c=c: c.verify_batch_identify(P, I, rand)) for v, c in builds.items()})
    rounds = [k for k in res["rows"] if k.startswith("recheck")]
    res["rounds_faster_by_more_than_parent_spread"] = all(-res["rows"][k]["this_minus_parent_ms"] > res["rows"][k]["parent_spread_ms"] for k in rounds)
    pass_row = res["rows"]["verify_batch_identify, 0 bad"]
    res["pass_path_within_parent_spread"] = pass_row["this_minus_parent_ms"] <= pass_row["parent_spread_ms"]
    print("every round faster than the parent by more than the parent's spread:", res["rounds_faster_by_more_than_parent_spread"])
    print("pass path not above the parent by more than the parent's spread:", res["pass_path_within_parent_spread"], flush=True)
    for b in staged.values():
        b.close()
    pctx.close()
    return res


if args.parent:
    res = against_parent(args.parent)
    ctx.close()
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)
    sys.exit(0)

res = {"n": n, "k": args.k, "reps": args.reps}
t, r = timed(lambda: ctx.verify_batch(P, I, rand))
assert r[0]
res["verify_batch_ms"] = round(t, 3)
print(f"verify_batch, 1024 good:           {t:8.3f} ms", flush=True)
res["identify"] = {}
for nb in (0, 1, 4, 32):
    bad = sorted(rnd.sample(range(n), nb))
    Q = spoiled(bad)
    t, r = timed(lambda: ctx.verify_batch_identify(Q, I, rand))
    assert [i for i in range(n) if r[1][i]] == bad and all(r[1][i] == -2 for i in bad)
    res["identify"][nb] = {"ms": round(t, 3), "range_checks": ctx.last_range_checks}
    print(f"verify_batch_identify, {nb:2d} bad:      {t:8.3f} ms   {ctx.last_range_checks:4d} range checks", flush=True)
Q = spoiled(sorted(rnd.sample(range(n), 4)))
t, r = timed(lambda: ctx.verify_each(Q, I))
res["verify_each_ms"] = round(t, 3)
print(f"verify_each, 1024 (4 bad):         {t:8.3f} ms", flush=True)
t, r = timed(lambda: ctx.verify_batch_identify(spoiled(range(n)), I, rand))
assert r[1] == [-2] * n
res["identify_all_bad_ms"] = round(t, 3); res["identify_all_bad_range_checks"] = ctx.last_range_checks
print(f"verify_batch_identify, all bad:    {t:8.3f} ms   {ctx.last_range_checks:4d} range checks", flush=True)

# one round of re-checks by its width: what the fan-out policy trades (rounds against checks per round)
b = h2v.Batch(ctx, n, N)
b.upload(d["proofs"], 1024, d["inst"], [N], b"".join(x.to_bytes(32, "little") for x in rand))
b.launch(); b.finish()
res["recheck_round_ms"] = {}
for width, size in ((1, 1024), (8, 128), (32, 32), (32, 1), (128, 1), (512, 1), (1024, 1)):
    ranges = [(i * (n // width), size) for i in range(width)] if size > 1 else [(i, 1) for i in range(width)]
    t, r = timed(lambda: b.recheck(ranges))
    assert all(r[0])
    res["recheck_round_ms"][f"{width}x{size}"] = round(t, 3)
    print(f"recheck {width:4d} ranges of {size:4d}:      {t:8.3f} ms", flush=True)
b.close()
ctx.close()
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
