"""What the draws of a seed cost, and what they save, on one MI355X:
   python tools/draws_probe.py --parent PATH [--k 14] [--groups 20] [--reps 7] [--out FILE]
PATH is a build of libh2v_amd.so made from the parent commit, loaded beside the in-tree one.  One process, at least 50 ms of warm-up
per variant, medians of --reps repetitions with the variants alternating inside each repetition.
 (a) k_expand_draws alone at 1024, 20 480 and 65 536 draws: device events around 200 back-to-back launches on one stream, per launch
     (launches of one stream do not overlap, so this is a launch's time once the queue is busy, not its latency from the host).
 (b) one launch of --groups x 1024 proofs resident in device memory, upload + launch + finish_groups through the Python mirror:
       seeded   this build:    upload_tensors(seed=...): the draws expanded on the batch's stream
       parent   parent build:  the draws made by h2v_random_scalars, copied to a tensor, upload_tensors(rand_tail=...)
       tensor   this build:    upload_tensors(rand_tail=...) with draws that were in device memory before the timed region
     and whether `seeded` is above `parent` by more than the spread (max - min) of `parent`'s own timings.
 (c) a shard's tail: 8192 proofs with a 65 536-draw tail (rank 0 of 8 x 8192, BASELINE config 3), the proofs resident:
       seeded    upload_tensors(seed=..., n_tail=65536)
       uploaded  the 2 MB of draws, already in host memory as a broadcast leaves them, copied to a tensor, upload_tensors(rand_tail=...)
Untimed: that the seeded launches return what the same draws return when given explicitly.
   python tools/draws_probe.py --trace
runs 20 launches of k_expand_draws at each of the three sizes and nothing else (no --parent needed), for a run of its own under
`rocprofv3 --kernel-trace --stats`: the kernel's own duration, which (a) cannot separate from the gap between two dispatches."""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
bench.hw_queue_env()
import torch
import halo2_verifier_amd as h2v
from halo2_verifier_amd import _lib, draws

ap = argparse.ArgumentParser()
ap.add_argument("--parent", default=None, help="a build of libh2v_amd.so from the parent commit")
ap.add_argument("--trace", action="store_true", help="only 20 launches of k_expand_draws per size, for a kernel trace")
ap.add_argument("--k", type=int, default=14)
ap.add_argument("--groups", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()

if args.trace:
    for count in (1024, 20480, 65536):
        out = torch.empty((count, 32), dtype=torch.uint8, device="cuda:0")
        for _ in range(20):
            draws.expand_into(bytes(range(32)), 0, out)
            torch.cuda.synchronize()
        print(f"{count} draws: 20 launches of {count // 16} workgroups")
    sys.exit(0)
if not args.parent:
    ap.error("--parent is required without --trace")

B, N, G = 1024, bench.N_PUBLIC, args.groups
n = B * G
SHARD, TAIL = 8192, 65536
d = bench.load_or_make_proofs(B, args.k, print)
raw = h2v.SerdeFormat.RawBytes
seed = bytes((37 * i + 11) % 256 for i in range(32))
dev = "cuda:0"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def context():
    return h2v.Context(h2v.ParamsKZG(d["params"], raw), h2v.VerifyingKey(d["vk"], raw))


parent = ctypes.CDLL(os.path.abspath(args.parent))
for name, (restype, argtypes) in _lib.SIGNATURES.items():
    fn = getattr(parent, name)
    fn.restype, fn.argtypes = restype, argtypes
assert not hasattr(parent, "h2v_draws_expand"), "--parent is not a build of the parent commit"
mine = _lib.load_library()
_lib._LIB = parent
try:
    pctx = context()
finally:
    _lib._LIB = mine
ctx = context()


def timed(variants, reps):
    """medians over `reps` repetitions, the variants alternating -> {name: (median, min, max)} in ms"""
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < bench.WARM_S * len(variants):
        for fn in variants.values():
            fn()
    ts = {v: [] for v in variants}
    for _ in range(reps):
        for v, fn in variants.items():
            t0 = time.perf_counter(); fn(); ts[v].append((time.perf_counter() - t0) * 1e3)
    return {v: (sorted(t)[len(t) // 2], min(t), max(t)) for v, t in ts.items()}


res = {"k": args.k, "reps": args.reps, "parent": args.parent}

# ---------------------------------------------------------------- (a) the kernel alone
say("(a) k_expand_draws alone: 200 back-to-back launches on one stream between two device events, per launch")
res["kernel_us"] = {}
stream = torch.cuda.Stream(device=dev)
for count in (1024, 20480, 65536):
    out = torch.empty((count, 32), dtype=torch.uint8, device=dev)
    with torch.cuda.stream(stream):
        t_end = time.perf_counter() + bench.WARM_S
        while time.perf_counter() < t_end:
            draws.expand_into(seed, 0, out)
        stream.synchronize()
        per = []
        for _ in range(args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(200):
                draws.expand_into(seed, 0, out)
            e1.record()
            e1.synchronize()
            per.append(e0.elapsed_time(e1) * 1e3 / 200)
    assert bytes(out[-1].cpu().numpy().tobytes()) == draws.draw(seed, count - 1)
    med = sorted(per)[len(per) // 2]
    res["kernel_us"][str(count)] = {"median": round(med, 2), "min": round(min(per), 2), "max": round(max(per), 2)}
    say(f"  {count:6d} draws  median {med:7.2f} us  min {min(per):.2f}  max {max(per):.2f}  ({count / med:8.1f} draws/us, {count // 16} waves)")

# ---------------------------------------------------------------- (b) the headline launch
proofs, inst = d["proofs"] * G, d["inst"] * G
t_proofs = torch.frombuffer(bytearray(proofs), dtype=torch.uint8).reshape(n, 1024).to(dev)
t_inst = torch.frombuffer(bytearray(inst), dtype=torch.uint8).reshape(n, 32 * N).to(dev)
t_rand = draws.expand_tensor(seed, 0, n, dev)
torch.cuda.synchronize()
batches = {"seeded": h2v.Batch(ctx, n, N, groups=G), "parent": h2v.Batch(pctx, n, N, groups=G), "tensor": h2v.Batch(ctx, n, N, groups=G)}


def run(b, **kw):
    b.upload_tensors(t_proofs, t_inst, [N], **kw)
    b.launch()
    return b.finish_groups(raw_statuses=True)


def parent_draws(count):
    buf = ctypes.create_string_buffer(32 * count)
    assert parent.h2v_random_scalars(buf, count) == 0
    return torch.frombuffer(buf, dtype=torch.uint8).reshape(count, 32).to(dev)


variants = {"seeded": lambda: run(batches["seeded"], seed=seed),
            "parent": lambda: run(batches["parent"], rand_tail=parent_draws(n)),
            "tensor": lambda: run(batches["tensor"], rand_tail=t_rand)}
want = variants["tensor"]()
assert all(want[0]) and want[1].count(0) == len(want[1])
assert variants["seeded"]() == want                     # the seed's draws, expanded, are the draws given
assert all(variants["parent"]()[0])                     # (its draws are the OS's: only the verdicts compare)
rows = timed(variants, args.reps)
say(f"(b) one launch of {G} x 1024 proofs resident in device memory: upload_tensors + launch + finish_groups")
for v, (med, lo, hi) in rows.items():
    say(f"  {v:8s} median {med:7.3f} ms  min {lo:.3f}  max {hi:.3f}  {n / med / 1e3:6.2f} M proofs/s")
spread = rows["parent"][2] - rows["parent"][1]
diff = rows["seeded"][0] - rows["parent"][0]
res["launch_ms"] = {v: {"median": round(m, 3), "min": round(lo, 3), "max": round(hi, 3)} for v, (m, lo, hi) in rows.items()}
res["parent_spread_ms"], res["seeded_minus_parent_ms"], res["seeded_within_parent_spread"] = round(spread, 3), round(diff, 3), diff <= spread
res["seeded_minus_tensor_ms"] = round(rows["seeded"][0] - rows["tensor"][0], 3)
say(f"  seeded - parent: {diff:+.3f} ms; the parent path's spread over its {args.reps} timings: {spread:.3f} ms; seeded - tensor: {res['seeded_minus_tensor_ms']:+.3f} ms")
say(f"  seeded not above the parent path by more than the parent path's spread: {diff <= spread}")
for b in batches.values():
    b.close()
del t_proofs, t_inst, t_rand

# ---------------------------------------------------------------- (c) a shard's tail
reps8 = SHARD // B
s_proofs = torch.frombuffer(bytearray(d["proofs"] * reps8), dtype=torch.uint8).reshape(SHARD, 1024).to(dev)
s_inst = torch.frombuffer(bytearray(d["inst"] * reps8), dtype=torch.uint8).reshape(SHARD, 32 * N).to(dev)
host_tail = bytearray(draws.expand(seed, 0, TAIL))      # what a broadcast of the draws leaves in host memory
torch.cuda.synchronize()
sb = {"seeded": h2v.Batch(ctx, SHARD, N), "uploaded": h2v.Batch(ctx, SHARD, N)}


def shard(b, **kw):
    b.upload_tensors(s_proofs, s_inst, [N], **kw)
    b.launch(with_pairing=False)
    return b.finish_groups(raw_statuses=True)


variants = {"seeded": lambda: shard(sb["seeded"], seed=seed, n_tail=TAIL),
            "uploaded": lambda: shard(sb["uploaded"], rand_tail=torch.frombuffer(host_tail, dtype=torch.uint8).reshape(TAIL, 32).to(dev))}
want = variants["uploaded"]()
assert want[1].count(0) == len(want[1]) and variants["seeded"]() == want
rows = timed(variants, args.reps)
say(f"(c) a shard of {SHARD} proofs with a {TAIL}-draw tail, resident proofs, no pairing: upload_tensors + launch + finish_groups")
for v, (med, lo, hi) in rows.items():
    say(f"  {v:8s} median {med:7.3f} ms  min {lo:.3f}  max {hi:.3f}")
res["shard_ms"] = {v: {"median": round(m, 3), "min": round(lo, 3), "max": round(hi, 3)} for v, (m, lo, hi) in rows.items()}
res["shard_seeded_minus_uploaded_ms"] = round(rows["seeded"][0] - rows["uploaded"][0], 3)
say(f"  seeded - uploaded: {res['shard_seeded_minus_uploaded_ms']:+.3f} ms ({32 * TAIL} bytes of draws not copied to the device)")
for b in sb.values():
    b.close()
ctx.close(); pctx.close()
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n" + json.dumps(res, indent=1) + "\n")
