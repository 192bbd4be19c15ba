"""Big-integer reference for feeding a finished batch's groups to a resident accumulator as legs (h2v_accumulator_process_batch), written
from the definition in include/h2v.h.  Nothing here ports a kernel: the products and sums are plain loops.

Group g holds the proofs [first_g, first_g + n_g) with draws r_{g,0} .. r_{g,n_g-1}; S_g is the group's own sum
sum_i (prod_{j > i} r_{g,j}) Guard_{g,i} and M_g the product of its draws:

    (L, R) <- (prod_g M_g) (L, R) + sum_g W_g S_g,     W_g = prod_{f > g} M_f

The functions take "points" of any additive group given by (add, mul, zero): integers mod r stand in for points in the CPU tests
(a Guard is then one scalar per side), the affine G1 of msm_reference in the kernel tests."""
from msm_reference import R

MAX_GROUPS = 512            # one workgroup of k_leg_weights


def offsets(sizes):
    """first_g of every group, and n behind them"""
    out = [0]
    for sz in sizes:
        assert sz >= 1
        out.append(out[-1] + sz)
    return out


def multipliers(draws):
    """mult[i] = the product of the draws behind i, for one group's draws"""
    out, m = [1] * len(draws), 1
    for i in range(len(draws) - 1, -1, -1):
        out[i] = m
        m = m * draws[i] % R
    return out


def group_multipliers(draws, sizes):
    """what an upload leaves in the batch: every proof's multiplier inside its own group"""
    off = offsets(sizes)
    assert off[-1] == len(draws)
    out = []
    for g in range(len(sizes)):
        out += multipliers(draws[off[g]:off[g + 1]])
    return out


def leg_products(first_draws, first_mults):
    """M_g as k_leg_weights forms it: the group's first draw times its first proof's multiplier"""
    return [d * m % R for d, m in zip(first_draws, first_mults)]


def leg_weights(Ms):
    """-> (prod_g M_g, [W_0 .. W_{G-1}]), W_g = prod_{f > g} M_f"""
    W, w = [1] * len(Ms), 1
    for g in range(len(Ms) - 1, -1, -1):
        W[g] = w
        w = w * Ms[g] % R
    return w, W


INT = (lambda a, b: (a + b) % R, lambda k, a: k * a % R, 0)     # integers mod r in place of points


def group_sum(draws, guards, grp=INT):
    """S = sum_i (prod_{j > i} r_j) Guard_i of one group: what a launch leaves for it"""
    add, mul, zero = grp
    s = zero
    for m, gd in zip(multipliers(draws), guards):
        s = add(s, mul(m, gd))
    return s


def process(acc, draws, guards, grp=INT):
    """one h2v_accumulator_process call, draw by draw: n x (scale by the draw, add the Guard), kzg/strategy.rs:125-136"""
    add, mul, _ = grp
    for r, gd in zip(draws, guards):
        acc = add(mul(r, acc), gd)
    return acc


def process_batch(acc, draws, guards, sizes, grp=INT):
    """the definition: -> (the accumulator afterwards, [(S_g, M_g)] as the journal's entries hold them)"""
    add, mul, _ = grp
    off = offsets(sizes)
    assert off[-1] == len(draws) == len(guards) and len(sizes) <= MAX_GROUPS
    mult = group_multipliers(draws, sizes)
    Ms = leg_products([draws[f] for f in off[:-1]], [mult[f] for f in off[:-1]])
    total, W = leg_weights(Ms)
    S = [group_sum(draws[off[g]:off[g + 1]], guards[off[g]:off[g + 1]], grp) for g in range(len(sizes))]
    out = mul(total, acc)
    for w, s in zip(W, S):
        out = add(out, mul(w, s))
    return out, list(zip(S, Ms))


def from_entries(entries, grp=INT):
    """the journal's invariant: sum_e W_e sum_e over entries [(sum, M)], W_e = prod_{f > e} M_f"""
    add, mul, zero = grp
    _, W = leg_weights([m for _, m in entries])
    out = zero
    for w, (s, _) in zip(W, entries):
        out = add(out, mul(w, s))
    return out


def legs_fold(records, pairs=None, slots=None):
    """k_accumulator_legs_fold over pairs of affine G1 points (None: the identity): records[i] = (left, right), record 0 the scaled
    accumulator.  -> ((left, right) = the sum of the records, {slot: pair} of the journal slots written: leg g's unscaled pair)"""
    import msm_reference as ref
    out = [None, None]
    for left, right in records:
        out[0], out[1] = ref.add(out[0], left), ref.add(out[1], right)
    written = {}
    if pairs is not None:
        assert len(pairs) == len(records) - 1
        written = {(slots[g] if slots is not None else g): pr for g, pr in enumerate(pairs)}
        assert len(written) == len(pairs)
    return tuple(out), written
