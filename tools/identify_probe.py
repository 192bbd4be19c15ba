"""Cost of finding the proofs that made a batch fail (h2v_verify_batch_identify) on ONE batch of 1024 proofs, against the batch alone
(h2v_verify_batch) and against SingleStrategy for every proof (h2v_verify_each); plus the cost of one round of re-checks by its width
(h2v_batch_recheck on a staged batch).  Median wall times of --reps runs, resident inputs:
   python tools/identify_probe.py [--k 14] [--reps 7] [--out FILE]
The proofs are the k = 14 pool bench.py caches (made here, from the same seeds, if no cache holds it).  A bad proof is a good one with
the sign of h2 flipped: it decodes and passes the transcript, only the pairing rejects it."""
import argparse, json, os, random, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
bench.hw_queue_env()
import halo2_verifier_amd as h2v

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=14)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()

n, N = 1024, bench.N_PUBLIC
d = bench.load_or_make_proofs(n, args.k, print)
ctx = h2v.Context(h2v.ParamsKZG(d["params"], h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(d["vk"], h2v.SerdeFormat.RawBytes))
P = [d["proofs"][1024 * i:1024 * (i + 1)] for i in range(n)]
I = [[[d["inst"][32 * (N * i + j):32 * (N * i + j + 1)] for j in range(N)]] for i in range(n)]
rnd = random.Random(2024)
rand = [rnd.randrange(1, R_MOD) for _ in range(n)]


def timed(fn):
    fn()   # warm-up: plans, scratch batch, workspaces
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); r = fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], r


def spoiled(bad):
    Q = list(P)
    for i in bad:
        b = bytearray(Q[i]); b[-1] ^= 0x40; Q[i] = bytes(b)
    return Q


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
