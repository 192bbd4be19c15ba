"""Cost of one accumulation over proofs of several VerifyingKeys (h2v_verify_batch_keys): V distinct vector-mul VKs at k = 8 over one
known-s setup (circuits.setup_vector_mul(8, n_mul) with a different n_mul per key), V in {1, 2, 4, 8}, 1024 proofs interleaved in call
order (proof i belongs to key i mod V).  For comparison: the single-key h2v_verify_batch on 1024 proofs of the first key, and the
per-proof path that AccumulatorStrategy.finalize took for several VKs before h2v_verify_batch_keys (one staged Batch per proof, its
record exported into a torch buffer, h2v_fold_check over all records) on 64 proofs, scaled to 1024.  Median wall times of --reps runs:
   python tools/multi_key_probe.py [--reps 7] [--out FILE]"""
import argparse, ctypes, json, os, random, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import circuits
import halo2_verifier_amd as h2v
from halo2_verifier_amd import _lib, distributed

R_MOD = circuits.R_MOD
ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()

N, POOL = 1024, 64                       # proofs per call; distinct proofs made per key (cycled)
N_MUL = [8, 7, 6, 5, 4, 3, 9, 10]        # one VK per n_mul
RAW = h2v.SerdeFormat.RawBytes
setups = [circuits.setup_vector_mul(8, m) for m in N_MUL]
assert all(s.params == setups[0].params for s in setups)
pools = [circuits.prove_vector_mul_batch(s, POOL, seed=100 + k, threads=16) for k, s in enumerate(setups)]
ctxs = [h2v.Context(h2v.ParamsKZG(s.params, RAW), h2v.VerifyingKey(s.vk, RAW)) for s in setups]
rnd = random.Random(2026)
rand = [rnd.randrange(1, R_MOD) for _ in range(N)]


def timed(fn):
    fn()   # warm-up: plans, scratch batches, workspaces
    ts = []
    for _ in range(args.reps):
        t0 = time.perf_counter(); r = fn(); ts.append((time.perf_counter() - t0) * 1e3)
    return sorted(ts)[len(ts) // 2], r


def calls(V, n):
    keys = [i % V for i in range(n)]
    P = [pools[k][0][(i // V) % POOL] for i, k in enumerate(keys)]
    I = [pools[k][1][(i // V) % POOL] for i, k in enumerate(keys)]
    return keys, P, I


def per_proof(keys, P, I, rb):
    """the removed per-proof path: a one-proof Batch per proof whose draw tail is the draws of proofs (i, n), one fold"""
    import torch
    n = len(P)
    records = torch.zeros(n * distributed.ACC_BYTES, dtype=torch.uint8, device="cuda:0")
    ok_all = True
    for i in range(n):
        flat = b"".join(v for col in I[i] for v in col)
        b = h2v.Batch(ctxs[keys[i]], 1, max(len(flat) // 32, 1))
        try:
            b.upload(P[i], len(P[i]), flat, [len(c) for c in I[i]], b"".join(rb[i:]))
            b.launch(with_pairing=False)
            b.export_accumulators(records.data_ptr() + i * distributed.ACC_BYTES)
            ok_all = ok_all and b.finish()[1] == [0]
        finally:
            b.close()
    ok = ctypes.c_int(0)
    _lib.check(_lib.load_library().h2v_fold_check(ctxs[0]._h, ctypes.c_void_p(records.data_ptr()), n, ctypes.byref(ok), None, None))
    return bool(ok.value) and ok_all


res = {"n": N, "k": 8, "reps": args.reps, "gpu_max_hw_queues": os.environ.get("GPU_MAX_HW_QUEUES"), "verify_batch_keys_ms": {}}
_, P, I = calls(1, N)
t, r = timed(lambda: ctxs[0].verify_batch(P, I, rand))
assert r[0]
res["single_key_verify_batch_ms"] = round(t, 3)
print(f"h2v_verify_batch, 1 key, {N} proofs:          {t:9.3f} ms", flush=True)
for V in (1, 2, 4, 8):
    keys, P, I = calls(V, N)
    t, r = timed(lambda: h2v.verify_batch_keys(ctxs[:V], keys, P, I, rand))
    assert r[0] and r[1] == [0] * N
    res["verify_batch_keys_ms"][V] = round(t, 3)
    print(f"h2v_verify_batch_keys, V = {V}, {N} proofs:   {t:9.3f} ms   ({t / res['single_key_verify_batch_ms']:.2f}x single key)", flush=True)
keys, P, I = calls(2, POOL)
rb = [r.to_bytes(32, "little") for r in rand[:POOL]]
t, ok = timed(lambda: per_proof(keys, P, I, rb))
assert ok
res["per_proof_path"] = {"proofs": POOL, "ms": round(t, 3), "ms_per_proof": round(t / POOL, 4), "scaled_to_n_ms": round(t / POOL * N, 1)}
print(f"per-proof path, V = 2, {POOL} proofs:           {t:9.3f} ms   ({t / POOL:.3f} ms per proof, {t / POOL * N:.0f} ms scaled to {N})", flush=True)
if args.out:
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
for c in ctxs:
    c.close()
for s in setups:
    s.free()
