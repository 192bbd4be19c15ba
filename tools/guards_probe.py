"""What the trait seam costs on the GPU: Guards from a CPU verify_proof fed to a resident accumulator, and checked one by one.
One process, one MI355X, host clocks around calls that end in a synchronise, after >= 50 ms of warm-up GPU work; the alternatives
alternate inside every repetition and every repetition is printed, so the spread is visible:
   python tools/guards_probe.py [--reps 7] [--out FILE]
The Guards are those of the k = 14 pool bench.py caches if .bench_cache/ holds it, else of 64 k = 8 vector-mul proofs, cycled to 1024
(made by the library's own h2v_guard_msm: this is a measurement, not a test).  The byte arrays of (a), (c), (d) and (f) are marshalled
outside the timed regions.
  8 legs of 1024 Guards, then finalize:
   (a) h2v_accumulator_process_guards per leg
   (b) h2v_accumulator_process over the same proofs: the whole-proof seam, for context
   (c) the route for the same terms without it: the multipliers applied on the host outside the timed region, one
       h2v_accumulator_add_msm per leg (no scale step: it does less than (a))
  1024 Guards, one verdict each:
   (d) h2v_guards_check_each
   (e) h2v_verify_each over the same proofs
   (f) per Guard 2 x h2v_msm_g1 + h2v_pairing_check, timed on 32 Guards and scaled by 32"""
import argparse, ctypes, json, os, random, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
bench.hw_queue_env()
import halo2_verifier_amd as h2v
from halo2_verifier_amd import verifier

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--out", default=None)
args = ap.parse_args()

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
RAW = h2v.SerdeFormat.RawBytes
K, n, N = 8, 1024, bench.N_PUBLIC

cached = any(os.path.exists(os.path.join(c, f"vm_k14_pub{N}_n{n}.proofs")) for c, _ in bench._cache_dirs())
if cached:
    d = bench.load_or_make_proofs(n, 14, print)
    pool = "k = 14 bench pool"
    vk, params = d["vk"], d["params"]
    P = [d["proofs"][1024 * i:1024 * (i + 1)] for i in range(n)]
    I = [[[d["inst"][32 * (N * i + j):32 * (N * i + j + 1)] for j in range(N)]] for i in range(n)]
else:
    import circuits
    s = circuits.setup_vector_mul(8, N)
    P0, I0 = circuits.prove_vector_mul_batch(s, 64, seed=77, threads=8)
    pool = "64 k = 8 vector-mul proofs, cycled"
    vk, params = s.vk, s.params
    P, I = [P0[i % 64] for i in range(n)], [I0[i % 64] for i in range(n)]

ctx = h2v.Context(h2v.ParamsKZG(params, RAW), h2v.VerifyingKey(vk, RAW))
lib = ctx._lib
made = {}
for i in range(n):
    if P[i] not in made:
        rc, g = ctx.guard_msm(P[i], I[i])
        assert rc == 0
        made[P[i]] = ((g["left_scalars"], g["left_bases"]), (g["right_scalars"], g["right_bases"]))
G = [made[p] for p in P]
rnd = random.Random(2026)
draws = [[rnd.randrange(1, R_MOD) for _ in range(n)] for _ in range(K)]
g_args = verifier._guards_args(G)
rand_bytes = [b"".join(r.to_bytes(32, "little") for r in leg) for leg in draws]


def scaled_leg(leg):
    """the leg's terms with the multipliers applied: what add_msm needs to add the same sum"""
    mult, run = [1] * n, 1
    for i in range(n - 1, -1, -1):
        mult[i] = run
        run = run * leg[i] % R_MOD
    sides = []
    for side in range(2):
        sc = [int.from_bytes(x, "little") * m % R_MOD for g, m in zip(G, mult) for x in g[side][0]]
        sides.append(verifier._channel((sc, [b for g in G for b in g[side][1]])))
    return sides[0] + sides[1]


add_args = [scaled_leg(leg) for leg in draws]
one_args = [[verifier._channel(side) for side in g] for g in G[:32]]


def run_a():
    acc = h2v.Accumulator(ctx)
    for j in range(K):
        verifier.check(lib.h2v_accumulator_process_guards(acc._h, *g_args, rand_bytes[j]))
    r = acc.finalize(); acc.close(); return r


def run_b():
    acc = h2v.Accumulator(ctx)
    for j in range(K):
        acc.process(ctx, None, P, I, draws[j])
    r = acc.finalize(); acc.close(); return r


def run_c():
    acc = h2v.Accumulator(ctx)
    for j in range(K):
        verifier.check(lib.h2v_accumulator_add_msm(acc._h, *add_args[j]))
    r = acc.finalize(); acc.close(); return r


def run_d():
    ok = (ctypes.c_int * n)()
    verifier.check(lib.h2v_guards_check_each(ctx._h, *g_args, ok))
    return list(ok)


def run_e():
    return [st == 0 for st in ctx.verify_each(P, I)]


def run_f():
    out = []
    xy, ident, ok = ctypes.create_string_buffer(128), ctypes.c_int(0), ctypes.c_int(0)
    for l, r in one_args:
        verifier.check(lib.h2v_msm_g1(ctx._h, l[0], l[1], l[2], xy, ctypes.byref(ident)))
        right = ctypes.create_string_buffer(64)
        verifier.check(lib.h2v_msm_g1(ctx._h, r[0], r[1], r[2], right, ctypes.byref(ident)))
        verifier.check(lib.h2v_pairing_check(ctx._h, xy.raw[:64], right.raw, ctypes.byref(ok)))
        out.append(ok.value)
    return out


runs = {"a": run_a, "b": run_b, "c": run_c, "d": run_d, "e": run_e, "f": run_f}
t0 = time.perf_counter()
first = {}
while time.perf_counter() - t0 < 0.05 or not first:   # warm-up: plans, workspaces, clocks
    first = {k: fn() for k, fn in runs.items()}
assert first["a"][0] is True and first["a"] == first["b"] and first["c"][0] is True, "the routes disagree"
assert all(first["d"]) and first["d"] == [1] * n and all(first["e"]) and all(first["f"])
ms = {k: [] for k in runs}
for _ in range(args.reps):
    for k, fn in runs.items():
        t = time.perf_counter(); fn(); ms[k].append((time.perf_counter() - t) * 1e3)
med = {k: sorted(v)[len(v) // 2] for k, v in ms.items()}
terms = (sum(len(g[0][0]) for g in G), sum(len(g[1][0]) for g in G))
lines = [f"guards_probe: {pool}; {n} Guards a leg with {terms[0]} left and {terms[1]} right terms; {K} legs; {args.reps} repetitions, milliseconds",
         "8 legs of 1024 Guards + finalize:"]
names = {"a": "(a) process_guards", "b": "(b) process (proof bytes)", "c": "(c) add_msm, multipliers on the host untimed", "d": "(d) guards_check_each",
         "e": "(e) verify_each (proof bytes)", "f": "(f) 2 x msm_g1 + pairing_check per Guard, 32 Guards"}
for k in "abc":
    lines.append(f"  {names[k]:48s} median {med[k]:9.3f}   all " + " ".join(f"{v:.3f}" for v in ms[k]))
lines.append(f"  (a) / (c) = {med['a'] / med['c']:.3f}   (a) / (b) = {med['a'] / med['b']:.3f}")
lines.append("1024 Guards, one verdict each:")
for k in "def":
    lines.append(f"  {names[k]:48s} median {med[k]:9.3f}   all " + " ".join(f"{v:.3f}" for v in ms[k]))
lines.append(f"  (f) scaled to 1024 Guards: {32 * med['f']:.3f}   (d) / (f scaled) = {med['d'] / (32 * med['f']):.4f}   (d) / (e) = {med['d'] / med['e']:.3f}")
text = "\n".join(lines) + "\n"
print(text, end="")
if args.out:
    with open(args.out, "w") as f:
        f.write(text)
ctx.close()
