"""What groups of unequal size cost (h2v_batch_set_group_sizes, h2v_verify_batches), on the benchmark's k = 14 proofs (1024 distinct,
cycled).  Three measurements, each a median of --reps runs after a warm-up of at least 50 ms of the same work:
  equal     one launch of 20 x 1024 proofs, inputs resident: launch + finish on a batch set up with set_groups(20), and the same on a
            batch set up with set_group_sizes([1024] * 20) — the same kernels over a GroupShape with offsets (csrc/batch.h), the groups' ends from
            the last-of-group marks — and upload + launch + finish of the same (the multipliers are computed at upload;
            --only-upload runs this leg alone, the form to put under a kernel trace for the kernels' own durations)
  skewed    [200, 1, 1, 1] x 8 (the window plan follows the largest problem of a launch) beside 32 equal groups of the same total
  batches   32 batches summing to 32 768 proofs, sizes from random.Random(2026) (SIZES below), from host bytes: one h2v_verify_batches
            call against 32 consecutive h2v_verify_batch calls (--only-consecutive: that leg alone, for a library without the new call)
            (through the Python mirror: its marshalling is inside both figures)
   python tools/ragged_probe.py [--reps 7] [--out FILE] [--only-consecutive | --only-upload]"""
import argparse, json, os, random, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
import halo2_verifier_amd as h2v

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
ap.add_argument("--only-consecutive", action="store_true")
ap.add_argument("--only-upload", action="store_true")
args = ap.parse_args()

WARM_S = 0.05
N_PUBLIC = bench.N_PUBLIC


def seeded_sizes(k=32, total=32768, seed=2026):
    """k sizes >= 1 summing to total: k - 1 distinct cut points drawn by random.Random(seed)"""
    cuts = sorted(random.Random(seed).sample(range(1, total), k - 1))
    return [b - a for a, b in zip([0] + cuts, cuts + [total])]


SIZES = seeded_sizes()
d = bench.load_or_make_proofs(1024, 14, lambda m: print(m, flush=True))
RAW = h2v.SerdeFormat.RawBytes
ctx = h2v.Context(h2v.ParamsKZG(d["params"], RAW), h2v.VerifyingKey(d["vk"], RAW))
PROOFS = [d["proofs"][1024 * i:1024 * i + 1024] for i in range(1024)]
INST = [[[d["inst"][32 * (N_PUBLIC * i + j):32 * (N_PUBLIC * i + j) + 32] for j in range(N_PUBLIC)]] for i in range(1024)]


def draws(n, salt=0):
    return [((i * 0x9e3779b97f4a7c15 + 0x1234567 + salt * 0x51ed27) % (1 << 250)) for i in range(1, n + 1)]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    while time.perf_counter() - t0 < WARM_S:
        fn()
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); r = fn(); ts.append((time.perf_counter() - t0) * 1e3)
    ts.sort()
    return ts[len(ts) // 2], ts[0], ts[-1], r


def resident(n, setup):
    """a batch of n cycled proofs, set up by `setup`, uploaded -> a function that launches and finishes it once"""
    b = h2v.Batch(ctx, n, N_PUBLIC)
    setup(b)
    reps = (n + 1023) // 1024
    host = ((d["proofs"] * reps)[:n * 1024], 1024, (d["inst"] * reps)[:n * 32 * N_PUBLIC], [N_PUBLIC], b"".join(r.to_bytes(32, "little") for r in draws(n)))
    b.upload(*host)

    def once(upload=False):
        if upload:
            b.upload(*host)
        b.launch()
        ok, st, left, right = b.finish_groups(raw_statuses=True)
        assert all(ok) and st.count(0) == len(st)
        return left, right
    return b, once


res = {"reps": args.reps, "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "sizes": SIZES}
if not args.only_consecutive:
    G, gs = 20, 1024
    b_eq, run_eq = resident(G * gs, lambda b: b.set_groups(G))
    b_rg, run_rg = resident(G * gs, lambda b: b.set_group_sizes([gs] * G))
    # alternately, so that both see the same clocks
    te, tr, ue, ur = [], [], [], []
    for _ in range(3):
        if not args.only_upload:
            te.append(timed(run_eq)); tr.append(timed(run_rg))
        ue.append(timed(lambda: run_eq(True))); ur.append(timed(lambda: run_rg(True)))
    up_eq, up_rg = sorted(t[0] for t in ue)[1], sorted(t[0] for t in ur)[1]
    assert ue[0][3] == ur[0][3], "the two paths disagree"
    res["equal_with_upload"] = {"set_groups_ms": round(up_eq, 4), "set_group_sizes_ms": round(up_rg, 4), "ratio": round(up_rg / up_eq, 4),
                                "set_groups_rounds_ms": [round(t[0], 4) for t in ue], "set_group_sizes_rounds_ms": [round(t[0], 4) for t in ur]}
    print(f"20 x 1024 upload + launch: set_groups {up_eq:.3f} ms, set_group_sizes {up_rg:.3f} ms, ratio {up_rg / up_eq:.3f}", flush=True)
    if args.only_upload:
        if args.out:
            with open(args.out, "w") as f:
                json.dump(res, f, indent=1)
        ctx.close()
        sys.exit(0)
    assert te[0][3] == tr[0][3] == ue[0][3], "the two paths disagree"
    eq, rg = sorted(t[0] for t in te)[1], sorted(t[0] for t in tr)[1]
    res["equal"] = {"set_groups_ms": round(eq, 4), "set_group_sizes_ms": round(rg, 4), "ratio": round(rg / eq, 4),
                    "set_groups_rounds_ms": [round(t[0], 4) for t in te], "set_group_sizes_rounds_ms": [round(t[0], 4) for t in tr]}
    print(f"20 x 1024 resident: set_groups {eq:.3f} ms, set_group_sizes {rg:.3f} ms, ratio {rg / eq:.3f}", flush=True)
    b_eq.close(); b_rg.close()

    skew = [200, 1, 1, 1] * 8
    n = sum(skew)
    b_sk, run_sk = resident(n, lambda b: b.set_group_sizes(skew))
    b_fl, run_fl = resident(n - n % 32, lambda b: b.set_groups(32))
    ts, tf = timed(run_sk), timed(run_fl)
    res["skewed"] = {"sizes": "[200, 1, 1, 1] x 8", "proofs": n, "ms": round(ts[0], 4), "equal_32_groups_proofs": n - n % 32, "equal_32_groups_ms": round(tf[0], 4)}
    print(f"[200, 1, 1, 1] x 8 ({n} proofs): {ts[0]:.3f} ms; 32 equal groups of {(n - n % 32) // 32}: {tf[0]:.3f} ms", flush=True)
    b_sk.close(); b_fl.close()

batches, rand, at = [], draws(sum(SIZES)), 0
for sz in SIZES:
    idx = [(at + j) % 1024 for j in range(sz)]
    batches.append(([PROOFS[i] for i in idx], [INST[i] for i in idx], rand[at:at + sz])); at += sz


def consecutive():
    return [ctx.verify_batch(p, i, r) for p, i, r in batches]


tc = timed(consecutive)
assert all(r[0] for r in tc[3])
res["batches"] = {"proofs": sum(SIZES), "consecutive_verify_batch_ms": round(tc[0], 3), "consecutive_min_max_ms": [round(tc[1], 3), round(tc[2], 3)]}
print(f"32 batches, {sum(SIZES)} proofs, consecutive h2v_verify_batch: {tc[0]:.2f} ms ({sum(SIZES) / tc[0] / 1e3:.3f} M proofs/s)", flush=True)
if not args.only_consecutive:
    tb = timed(lambda: ctx.verify_batches([(p, i) for p, i, _ in batches], rand))
    assert tb[3] == tc[3], "h2v_verify_batches disagrees with the consecutive calls"
    res["batches"].update({"verify_batches_ms": round(tb[0], 3), "verify_batches_min_max_ms": [round(tb[1], 3), round(tb[2], 3)], "speedup": round(tc[0] / tb[0], 3)})
    print(f"one h2v_verify_batches call: {tb[0]:.2f} ms ({sum(SIZES) / tb[0] / 1e3:.3f} M proofs/s), {tc[0] / tb[0]:.2f}x", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
ctx.close()
