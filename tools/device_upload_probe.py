"""What an upload from device memory (h2v_batch_upload_device) costs at the headline launch, 20 groups of 1024 proofs of the k = 14 pool,
against the ways in that start from host memory:
   python tools/device_upload_probe.py --parent PATH [--k 14] [--groups 20] [--reps 7] [--out FILE]
PATH is a build of libh2v_amd.so made from the parent commit, loaded beside the in-tree one.  One MI355X, one process, at least 50 ms
of warm-up; medians of --reps repetitions with the variants alternating inside each repetition:
   device    this build:    upload_device (inputs and draws in device memory) + launch + finish_groups
   upload    parent build:  upload (host memory) + launch + finish_groups
   overlap   parent build:  upload_launch (the copy hidden behind the decompression) + finish_groups
   resident  this build:    launch + finish_groups on inputs uploaded before the timed region
and, untimed, that all of them return the same results.  Prints each variant's median and min .. max, the parent's spread for
`upload`, and whether `device` is above `upload` by more than that spread."""
import argparse, ctypes, json, os, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
bench.hw_queue_env()
import torch
import halo2_verifier_amd as h2v
from halo2_verifier_amd import _lib

ap = argparse.ArgumentParser()
ap.add_argument("--parent", required=True, help="a build of libh2v_amd.so from the parent commit")
ap.add_argument("--k", type=int, default=14)
ap.add_argument("--groups", type=int, default=20)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()

B, N, G = 1024, bench.N_PUBLIC, args.groups
n = B * G
d = bench.load_or_make_proofs(B, args.k, print)
proofs, inst = d["proofs"] * G, d["inst"] * G
rand = b"".join(((i * 0x9e3779b97f4a7c15 + 0x1234567) % (1 << 250)).to_bytes(32, "little") for i in range(1, n + 1))
raw = h2v.SerdeFormat.RawBytes


def context():
    return h2v.Context(h2v.ParamsKZG(d["params"], raw), h2v.VerifyingKey(d["vk"], raw))


parent = ctypes.CDLL(os.path.abspath(args.parent))   # (a parent build lacks the newer symbols)
for name, (restype, argtypes) in _lib.SIGNATURES.items():
    if hasattr(parent, name):
        fn = getattr(parent, name)
        fn.restype, fn.argtypes = restype, argtypes
assert not hasattr(parent, "h2v_batch_upload_device"), "--parent is not a build of the parent commit"
mine = _lib.load_library()
_lib._LIB = parent
try:
    pctx = context()
finally:
    _lib._LIB = mine
ctx = context()

dev = "cuda:0"
t_proofs = torch.frombuffer(bytearray(proofs), dtype=torch.uint8).reshape(n, 1024).to(dev)
t_inst = torch.frombuffer(bytearray(inst), dtype=torch.uint8).reshape(n, 32 * N).to(dev)
t_rand = torch.frombuffer(bytearray(rand), dtype=torch.uint8).reshape(n, 32).to(dev)
torch.cuda.synchronize()

batches = {v: h2v.Batch(c, n, N, groups=G) for v, c in (("device", ctx), ("upload", pctx), ("overlap", pctx), ("resident", ctx))}
batches["resident"].upload(proofs, 1024, inst, [N], rand)


def device():
    b = batches["device"]
    b.upload_device(t_proofs.data_ptr(), n, 1024, t_inst.data_ptr(), [N], t_rand.data_ptr(), n)
    b.launch()
    return b.finish_groups(raw_statuses=True)


def upload():
    b = batches["upload"]
    b.upload(proofs, 1024, inst, [N], rand)
    b.launch()
    return b.finish_groups(raw_statuses=True)


def overlap():
    b = batches["overlap"]
    b.upload_launch(proofs, 1024, inst, [N], rand)
    return b.finish_groups(raw_statuses=True)


def resident():
    b = batches["resident"]
    b.launch()
    return b.finish_groups(raw_statuses=True)


variants = {"device": device, "upload": upload, "overlap": overlap, "resident": resident}
want = resident()
assert all(want[0]) and want[1].count(0) == len(want[1])
for v, fn in variants.items():
    assert fn() == want, v           # every way in gives the same verdicts, statuses and channels
t0 = time.perf_counter()
while time.perf_counter() - t0 < bench.WARM_S * 4:   # (each variant for at least 50 ms)
    for fn in variants.values():
        fn()
ts = {v: [] for v in variants}
for _ in range(args.reps):
    for v, fn in variants.items():
        t0 = time.perf_counter(); fn(); ts[v].append((time.perf_counter() - t0) * 1e3)

res = {"n": n, "groups": G, "k": args.k, "reps": args.reps, "parent": args.parent, "rows": {}}
for v, t in ts.items():
    res["rows"][v] = {"median_ms": round(sorted(t)[len(t) // 2], 3), "min_ms": round(min(t), 3), "max_ms": round(max(t), 3),
                      "mproofs_per_s": round(n / sorted(t)[len(t) // 2] / 1e3, 2)}
    r = res["rows"][v]
    print(f"{v:9s} {r['median_ms']:7.3f} ms  [{r['min_ms']:.3f} .. {r['max_ms']:.3f}]  {r['mproofs_per_s']:6.2f} M proofs/s", flush=True)
spread = res["rows"]["upload"]["max_ms"] - res["rows"]["upload"]["min_ms"]
diff = res["rows"]["device"]["median_ms"] - res["rows"]["upload"]["median_ms"]
res["parent_upload_spread_ms"], res["device_minus_parent_upload_ms"] = round(spread, 3), round(diff, 3)
res["device_within_parent_spread"] = diff <= spread
res["ingest_over_resident_ms"] = round(res["rows"]["device"]["median_ms"] - res["rows"]["resident"]["median_ms"], 3)
print(f"device - parent's upload: {diff:+.3f} ms; the parent's spread over its {args.reps} timings: {spread:.3f} ms; "
      f"device - resident: {res['ingest_over_resident_ms']:+.3f} ms")
print("device not above the parent's upload by more than the parent's spread:", res["device_within_parent_spread"], flush=True)
for b in batches.values():
    b.close()
ctx.close(); pctx.close()
print(json.dumps(res))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(f"{v:9s} median {r['median_ms']:7.3f} ms  min {r['min_ms']:.3f}  max {r['max_ms']:.3f}  {r['mproofs_per_s']:6.2f} M proofs/s"
                          for v, r in res["rows"].items()) + "\n" + json.dumps(res, indent=1) + "\n")
