"""What holding terms on the GPU buys: the resident MSM object against the one-shot entry points of the PARENT commit's library.
One process, one MI355X, host clocks around calls that end in a synchronise, after >= 50 ms of warm-up GPU work and one untimed call
of every variant at every size; the variants alternate inside every repetition and every repetition is printed, so the spread is
visible.  Medians of 7.
   python tools/msm_object_probe.py --parent-lib PATH/libh2v_amd.so [--reps 7] [--max-log2 20] [--out FILE]
--parent-lib: libh2v_amd.so built from the parent commit (it is loaded beside this tree's library; both serve their own contexts).
  (1) eval: a resident object of 2^14 .. 2^20 terms (MSMKZG.eval: no upload, no conversion) against the parent's h2v_msm_g1 over the same
      host bytes.  The bases are the 256 SRS points of tests/golden/kzg_bn254_8.srs cycled, so the exact point is the CPU oracle's 256-term
      MSM of the per-base sums of the scalars; both results are checked against it before a time counts.
  (2) check: dual_check_many over 512 resident single-Guard DualMSM objects against the parent's h2v_guards_check_each over the same 512
      Guards from host bytes (marshalled outside the timed region); the verdict lists are compared.
Gate, per line: the resident median is not above the parent's median by more than the parent's own spread, (max - min) / median of its
timings at that size; the spread is printed beside the ratio.  A line that loses is reported as measured."""
import argparse, ctypes, os, random, sys, time
sys.path.insert(0, "."); sys.path.insert(0, "tests")
import bench
bench.hw_queue_env()
import halo2_verifier_amd as h2v
from halo2_verifier_amd import _lib, verifier
import circuits, oracle_lib, srs_util
from srs_util import g1_xy

ap = argparse.ArgumentParser()
ap.add_argument("--parent-lib", required=True)
ap.add_argument("--reps", type=int, default=7)
ap.add_argument("--max-log2", type=int, default=20)
ap.add_argument("--out", default=None)
args = ap.parse_args()

R_MOD = srs_util.R_MOD
RAW = h2v.SerdeFormat.RawBytes
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def median(v):
    return sorted(v)[len(v) // 2]


def timed(fn):
    t0 = time.perf_counter()
    r = fn()
    return (time.perf_counter() - t0) * 1e3, r


def report(name_new, name_old, t_new, t_old):
    m_new, m_old = median(t_new), median(t_old)
    spread = (max(t_old) - min(t_old)) / m_old
    ratio = m_new / m_old
    say(f"  {name_new:<34} median {m_new:9.3f}   all " + " ".join(f"{t:.3f}" for t in t_new))
    say(f"  {name_old:<34} median {m_old:9.3f}   all " + " ".join(f"{t:.3f}" for t in t_old))
    say(f"  resident / parent = {ratio:.3f}   parent's spread (max - min) / median = {spread:.3f}   gate: {'holds' if ratio <= 1 + spread else 'LOSES'}")


# the parent's library beside this tree's: the entry points the probe calls, with the signatures of _lib.py
parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
for name in ("h2v_ctx_create", "h2v_ctx_destroy", "h2v_msm_g1", "h2v_guards_check_each", "h2v_last_error"):
    fn = getattr(parent, name)
    fn.restype, fn.argtypes = _lib.SIGNATURES[name]
assert not hasattr(parent, "h2v_msm_create"), "--parent-lib already has the resident MSM object: not the parent commit's library"


def parent_ctx(params, vk=None):
    h = ctypes.c_void_p()
    rc = parent.h2v_ctx_create(params, len(params), int(RAW), vk, len(vk) if vk else 0, int(RAW) if vk else 0, 0, ctypes.byref(h))
    assert rc == 0, parent.h2v_last_error()
    return h


srs = srs_util.load_srs(os.path.join(ROOT, "tests", "golden", "kzg_bn254_8.srs"))
oracle = oracle_lib.load()
pts = [g1_xy(p) for p in srs.g]
say(f"msm_object_probe: {args.reps} repetitions, milliseconds; variants alternate inside every repetition")

# warm-up: >= 50 ms of GPU work on this tree's library (clocks, code objects)
ctx = h2v.Context(h2v.ParamsKZG(srs.params_raw, RAW))
rnd = random.Random(2027)
t0 = time.perf_counter()
while time.perf_counter() - t0 < 0.2:
    ctx.msm_g1([rnd.randrange(R_MOD) for _ in range(4096)], [pts[i % 256] for i in range(4096)])

say("(1) eval of 2^k terms, the 256 SRS bases cycled:")
pctx = parent_ctx(srs.params_raw)
for k in range(14, args.max_log2 + 1):
    n = 1 << k
    scalars = [rnd.randrange(R_MOD) for _ in range(n)]
    sb = b"".join(s.to_bytes(32, "little") for s in scalars)
    bb = b"".join(pts) * (n // 256)
    exp = oracle_lib.g1_msm(oracle, [sum(scalars[j::256]) % R_MOD for j in range(256)], pts)
    m = h2v.MSMKZG(ctx)
    verifier.check(ctx._lib.h2v_msm_append_terms(m._h, sb, bb, n))
    out = ctypes.create_string_buffer(64)
    ident = ctypes.c_int(0)

    def old():
        assert parent.h2v_msm_g1(pctx, sb, bb, n, out, ctypes.byref(ident)) == 0
        return out.raw

    new = m.eval
    assert new() == exp and old() == exp   # (and the untimed first call of both)
    t_new, t_old = [], []
    for rep in range(args.reps):
        for which in ((0, 1) if rep % 2 == 0 else (1, 0)):
            t, r = timed(new if which == 0 else old)
            assert r == exp
            (t_new if which == 0 else t_old).append(t)
    say(f" 2^{k} = {n} terms")
    report("resident MSMKZG.eval", "parent h2v_msm_g1 (host bytes)", t_new, t_old)
    m.close()
parent.h2v_ctx_destroy(pctx)
ctx.close()

say("(2) 512 Guards of k = 8 vector-mul proofs (64 proofs cycled), one verdict each:")
K = 512
s = circuits.setup_vector_mul(8, bench.N_PUBLIC)
P0, I0 = circuits.prove_vector_mul_batch(s, 64, seed=77, threads=8)
ctx = h2v.Context(h2v.ParamsKZG(s.params, RAW), h2v.VerifyingKey(s.vk, RAW))
made = []
for p, inst in zip(P0, I0):
    rc, g = ctx.guard_msm(p, inst)
    assert rc == 0
    made.append(((g["left_scalars"], g["left_bases"]), (g["right_scalars"], g["right_bases"])))
G = [made[i % 64] for i in range(K)]
g_args = verifier._guards_args(G)
duals = []
for g in G:
    d = h2v.DualMSM(ctx)
    d.add_msm(g)
    duals.append(d)
lefts = (ctypes.c_void_p * K)(*[d.left._h for d in duals])
rights = (ctypes.c_void_p * K)(*[d.right._h for d in duals])
ok_new, ok_old = (ctypes.c_int * K)(), (ctypes.c_int * K)()
pctx = parent_ctx(s.params, s.vk)


def new():
    verifier.check(ctx._lib.h2v_dual_msm_check_many(lefts, rights, K, ok_new, None, None))
    return list(ok_new)


def old():
    assert parent.h2v_guards_check_each(pctx, *g_args, ok_old) == 0
    return list(ok_old)


assert new() == old() == [1] * K
t_new, t_old = [], []
for rep in range(args.reps):
    for which in ((0, 1) if rep % 2 == 0 else (1, 0)):
        t, r = timed(new if which == 0 else old)
        assert r == [1] * K
        (t_new if which == 0 else t_old).append(t)
say(f" {K} Guards, {sum(g_args[1])} left and {sum(g_args[2])} right terms")
report("resident dual_check_many", "parent h2v_guards_check_each", t_new, t_old)
for d in duals:
    d.close()
parent.h2v_ctx_destroy(pctx)
ctx.close()
s.free()
if args.out:
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")
