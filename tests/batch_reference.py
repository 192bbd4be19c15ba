"""Exact reference for AccumulatorStrategy batches of any size, from the linearity of the accumulation.

For one group of proofs 0..n-1 with draws d_0..d_{n-1} (kzg/strategy.rs:125-140, msm.rs:173-176):

    left = sum_i m_i L_i,   right = sum_i m_i R_i,   m_i = prod_{j > i} d_j  (mod r)

where (L_i, R_i) is proof i's own Guard evaluated with multiplier 1 (the CPU oracle's Guard, then its G1 MSM), and proofs with a
non-zero status are left out.  The verdict is the oracle's pairing check of (left, right) and no non-zero status.  So a batch costs one
oracle Guard per DISTINCT proof (cached for the session) and one G1 MSM with one term per distinct proof, whose coefficient is the sum
of that proof's multipliers — where circuits.oracle_verify_batch restates the reference's O(n^2) scaling.

Under SHPLONK the left channel of a Guard is one term with scalar 1, so the left-channel scalars of a batch's pooled MSM ARE the
multipliers: draws_for() programs any non-zero multiplier sequence (whose last entry per group is 1).  A zero draw zeroes the
multipliers of every earlier proof of its group; the first draw of a group scales nothing (except a seed: see expected())."""
import oracle_lib
import circuits
from circuits import R_MOD

ZERO = bytes(64)   # the identity at the library's boundary (x | y all zero)

_SINGLE = {}


def _int(d):
    return int.from_bytes(d, "little") if isinstance(d, (bytes, bytearray)) else int(d)


def multipliers(draws, groups=1):
    """Per-group suffix products of the draws: group g owns proofs [g n/G, (g+1) n/G) (h2v_batch_set_groups).  -> list of ints mod r"""
    n = len(draws)
    assert n % groups == 0, (n, groups)
    gs = n // groups
    out = [0] * n
    for g in range(groups):
        run = 1
        for i in range(g * gs + gs - 1, g * gs - 1, -1):
            out[i] = run
            run = run * _int(draws[i]) % R_MOD
    return out


def draws_for(mults, groups=1, first=1):
    """The inverse of multipliers(): draws whose suffix products are `mults` (non-zero; the last of each group 1).  d_{i+1} = m_i / m_{i+1};
    the first draw of every group scales nothing and is `first`."""
    n = len(mults)
    assert n % groups == 0, (n, groups)
    gs = n // groups
    d = [0] * n
    for g in range(groups):
        lo = g * gs
        assert mults[lo + gs - 1] % R_MOD == 1, "the last multiplier of a group is always 1"
        d[lo] = first
        for i in range(lo, lo + gs - 1):
            assert mults[i + 1] % R_MOD, "a multiplier before the last one of its group is 0: not programmable by draws"
            d[i + 1] = mults[i] * pow(mults[i + 1], -1, R_MOD) % R_MOD
    return d


def _key(setup, proof, instances):
    inst = b"".join(b"".join(circuits.le32(v) if not isinstance(v, (bytes, bytearray)) else bytes(v) for v in col) for col in instances)
    return (setup.vk, setup.params, setup.multiopen, setup.transcript, setup.circuit_instances, bytes(proof), inst,
            tuple(len(col) for col in instances))


def single(setup, proof, instances):
    """(status, L_i, R_i): proof i's Guard by the oracle, both channels evaluated with multiplier 1 (None when status != 0).  Cached."""
    k = _key(setup, proof, instances)
    hit = _SINGLE.get(k)
    if hit is None:
        rc, g = circuits.oracle_guard(setup, proof, instances)
        if rc != 0:
            hit = (rc, None, None)
        else:
            L = setup.L
            ev = lambda sc, bs: oracle_lib.g1_msm(L, [int.from_bytes(x, "little") for x in sc], bs) if sc else ZERO
            hit = (0, ev(g["left_scalars"], g["left_bases"]), ev(g["right_scalars"], g["right_bases"]))
        _SINGLE[k] = hit
    return hit


def _combine(setup, coef):
    """sum coef[pt] pt over evaluated points (zero coefficients and identity points dropped)"""
    terms = [(c % R_MOD, pt) for pt, c in coef.items() if c % R_MOD and pt != ZERO]
    if not terms:
        return ZERO
    return oracle_lib.g1_msm(setup.L, [c for c, _ in terms], [pt for _, pt in terms])


def _accumulate(setup, items, mults, extra=()):
    """-> (statuses, left, right) of sum_i mults[i] (L_i, R_i) + sum (c, Lpt, Rpt) in extra"""
    cl, cr, statuses = {}, {}, []
    for (s, proof, inst), m in zip(items, mults):
        rc, L, R = single(s, proof, inst)
        statuses.append(rc)
        if rc == 0:
            cl[L] = cl.get(L, 0) + m
            cr[R] = cr.get(R, 0) + m
    for c, L, R in extra:
        cl[L] = cl.get(L, 0) + c
        cr[R] = cr.get(R, 0) + c
    return statuses, _combine(setup, cl), _combine(setup, cr)


def expected(items, draws, seed=None, setup=None):
    """One AccumulatorStrategy batch -> (ok, statuses, left_xy, right_xy) as Context.verify_batch returns it.
    items: [(setup, proof, instances)] in call order (setups may differ: several keys over the same params).
    seed: (left_xy, right_xy) of a starting accumulator (AccumulatorStrategy::with): it is scaled by the product of ALL draws, the
    first one included.  setup: whose params check the pairing when items is empty."""
    items = list(items)
    extra = ()
    if seed is not None:
        M = 1
        for d in draws:
            M = M * _int(d) % R_MOD
        extra = [(M, seed[0], seed[1])]
    if setup is None:
        setup = items[0][0]
    statuses, left, right = _accumulate(setup, items, multipliers(draws), extra)
    ok = not any(statuses) and circuits.oracle_pairing_check(setup, left, right)
    return ok, statuses, left, right


def expected_groups(items, draws, groups):
    """A grouped launch -> (group_ok[G], statuses[n], left_xy[G], right_xy[G]) as Batch.finish_groups returns it."""
    items = list(items)
    n = len(items)
    assert n % groups == 0
    gs = n // groups
    oks, statuses, lefts, rights = [], [], [], []
    for g in range(groups):
        ok, st, left, right = expected(items[g * gs:(g + 1) * gs], draws[g * gs:(g + 1) * gs])
        oks.append(ok); statuses += st; lefts.append(left); rights.append(right)
    return oks, statuses, lefts, rights


def expected_range(items, draws, first, count, groups=1):
    """What h2v_batch_recheck checks for proofs [first, first + count) of a launch: sum over the range of m_i (L_i, R_i) with the
    launch's own (per-group) multipliers, failed proofs contributing nothing.  -> (ok, left_xy, right_xy)"""
    items = list(items)
    mults = multipliers(draws, groups)
    _, left, right = _accumulate(items[first][0], items[first:first + count], mults[first:first + count])
    return circuits.oracle_pairing_check(items[first][0], left, right), left, right


# ---- programmed draws

# the GLV lattice of csrc/msm.hip glv_decompose: (a1, b1) and (a2, b2) with a_i + b_i lambda = 0 (mod r); g1, g2 the rounded
# 2^256 b2 / r and -2^256 b1 / r.  Restated only to FIND edge scalars; the oracle alone decides expected values.
GLV_A1, GLV_A2, GLV_B2 = 0x6f4d8248eeb859fc8211bbeb7d4f1128, 0x89d3256894d213e3, 0x6f4d8248eeb859fd0be4e1541221250b
GLV_B1 = -GLV_A2
GLV_G1, GLV_G2 = 0x24ccef014a773d2d25398fd0300ff6565, 0x2d91d232ec7e0b3d7
LAMBDA = GLV_A1 * pow(GLV_A2, -1, R_MOD) % R_MOD   # a1 + b1 lambda = 0  (lambda^2 + lambda + 1 = 0: the eigenvalue of phi)


def glv_split(k):
    """(k1, k2), signed, k = k1 + k2 lambda (mod r), as glv_decompose computes them"""
    c1, c2 = (k * GLV_G1) >> 256, (k * GLV_G2) >> 256
    return k - c1 * GLV_A1 - c2 * GLV_A2, -c1 * GLV_B1 - c2 * GLV_B2


def glv_edge_scalars(samples=3000, seed=5):
    """Scalars whose GLV halves are largest in magnitude, and the pairs on both sides of a step of the rounded quotient c1 (where a half
    changes sign): a short deterministic search."""
    import random
    rnd = random.Random(seed)
    cand = [rnd.randrange(1, R_MOD) for _ in range(samples)]
    steps = []
    for _ in range(8):                      # k at which c1 = floor(k g1 / 2^256) steps: k1 jumps by a1
        j = rnd.randrange(1, GLV_G1 >> 2)
        k = -((-j << 256) // GLV_G1)
        if 1 < k < R_MOD - 1:
            steps += [k - 1, k]
    halves = [(k, glv_split(k)) for k in cand + steps]
    big1 = sorted(halves, key=lambda t: -abs(t[1][0]))[:3]
    big2 = sorted(halves, key=lambda t: -abs(t[1][1]))[:3]
    return [k for k, _ in big1 + big2] + steps


def single_digit_scalars():
    """Values with one non-zero signed digit for every window width the MSM plan picks (c = 2 .. 15): below 2^126 the GLV split is
    (k, 0), so d 2^(c w) with d = 1, 2^(c-1) (the largest positive digit) and 2^(c-1) + 1 (a negative digit, carry into window w+1)."""
    out = set()
    for c in range(2, 16):
        for w in (0, 1, (125 // c) // 2, 125 // c - 1):
            for d in (1, 1 << (c - 1), (1 << (c - 1)) + 1):
                v = d << (c * w)
                if 0 < v < 1 << 126:
                    out.add(v)
    return sorted(out)


def programmed_values():
    """The edge scalars of the GLV split and the signed recoding, as multipliers (all non-zero)."""
    v = [1, 2, R_MOD - 1, R_MOD - 2, (R_MOD - 1) // 2, (R_MOD + 1) // 2]
    for k in (1, 63, 64, 127, 128, 129, 252, 253):
        v += [1 << k, R_MOD - (1 << k)]
    v += [LAMBDA, R_MOD - LAMBDA, LAMBDA + 1, LAMBDA - 1]
    v += glv_edge_scalars()
    v += single_digit_scalars()
    return [x % R_MOD for x in v]


def programmed_multipliers(n, groups=1, reps=3, offset=0):
    """n multipliers cycling programmed_values(), each value `reps` times in a row (equal scalars share buckets); the last of every group 1"""
    vals = programmed_values()
    gs = n // groups
    m = []
    for g in range(groups):
        m += [vals[((offset + i) // reps) % len(vals)] for i in range(gs - 1)] + [1]
    return m


def pattern_draws(kind, n, seed=0, k=None):
    """Draws of one group of n proofs: 'random' (uniform, non-zero), 'ones' (every multiplier 1), 'alternating' (every draw r - 1:
    multipliers +-1), 'zero_at' (random, with a zero draw at k: the proofs before k drop out), 'programmed' (multipliers = programmed values)."""
    import random
    rnd = random.Random(seed)
    if kind == "random":
        return [rnd.randrange(1, R_MOD) for _ in range(n)]
    if kind == "ones":
        return [1] * n
    if kind == "alternating":
        return [R_MOD - 1] * n
    if kind == "zero_at":
        d = [rnd.randrange(1, R_MOD) for _ in range(n)]
        d[k] = 0
        return d
    if kind == "programmed":
        return draws_for(programmed_multipliers(n, offset=seed))
    raise ValueError(kind)
