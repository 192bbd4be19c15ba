"""What a Guard of a batch is (include/h2v_guards.h), in Python integers, and a pure model of the kernel that gathers it.

The definition.  A launch of proofs in groups with draws d (one per proof) leaves, for proof p, the terms of its own GuardKZG with
every scalar multiplied by mult[p] = the product of the draws BEHIND p inside its group (kzg/strategy.rs:129, msm.rs:173-183: what the
reference's msm_accumulator holds for that proof once its whole group has been processed).  expected() builds it from the CPU oracle's
Guard of each proof (circuits.oracle_guard):
  SHPLONK  the oracle's lists, term for term;
  GWC      the oracle's per-query list merged: a base that occurs several times is reported once, at its first appearance, with its
           scalars summed (the plan's MSM order, Scalars::term in csrc/vkplan.hip);
  a proof with a status has no Guard: T_L and T_R zero scalars under the all-zero base.

The model.  gather() restates k_guards_gather (csrc/guards_out.hip) over programmed arrays: an order table of (kind, index) pairs,
slot scalars [p][slot], VK-wide scalars [j][p], points [p][slot] + VK-wide bases, rank-coded status words."""
import circuits
from circuits import R_MOD

ZERO = bytes(64)

# the device's rank-coded status words (csrc/batch.h) -> the ABI's codes (status_decode)
DEV_STATUS = {0: 0, -40: -1, -30: -5, -20: -7, -10: -4}


def decode_status(dev):
    return DEV_STATUS.get(dev, dev)


def _int(v):
    return int.from_bytes(v, "little") if isinstance(v, (bytes, bytearray)) else int(v)


def group_multipliers(draws, sizes):
    """mult[p] = the product of the draws behind p inside its group; groups of `sizes` proofs in upload order"""
    assert sum(sizes) == len(draws), (sizes, len(draws))
    out, lo = [0] * len(draws), 0
    for sz in sizes:
        run = 1
        for i in range(lo + sz - 1, lo - 1, -1):
            out[i] = run
            run = run * _int(draws[i]) % R_MOD
        lo += sz
    return out


def merge_first_appearance(scalars, bases):
    """every base once, where it first appears, with the sum of its scalars (mod r)"""
    at, out_s, out_b = {}, [], []
    for sc, b in zip(scalars, bases):
        if b in at:
            out_s[at[b]] = (out_s[at[b]] + sc) % R_MOD
        else:
            at[b] = len(out_b)
            out_s.append(sc % R_MOD)
            out_b.append(b)
    return out_s, out_b


def raw_guard(setup, proof, instances):
    """(status, guard): the oracle's Guard of one proof as integer scalars, in the batch form's term order (None with a status)"""
    rc, g = circuits.oracle_guard(setup, proof, instances)
    if rc != 0:
        return rc, None
    ints = lambda xs: [int.from_bytes(x, "little") for x in xs]
    left = (ints(g["left_scalars"]), list(g["left_bases"]))
    right = (ints(g["right_scalars"]), list(g["right_bases"]))
    if setup.multiopen == circuits.GWC:
        right = merge_first_appearance(*right)
    return 0, dict(left_scalars=left[0], left_bases=left[1], right_scalars=right[0], right_bases=right[1])


def expected(setup, proofs, instances, rand, sizes, shape=None):
    """One dict per proof: left_scalars / right_scalars (ints), left_bases / right_bases (64 bytes each), mult (int), status.
    rand: one draw per proof; sizes: the groups' sizes.  shape: (T_L, T_R) for an upload none of whose proofs has a Guard."""
    mult = group_multipliers(rand, sizes)
    raws = [raw_guard(setup, p, i) for p, i in zip(proofs, instances)]
    for rc, g in raws:
        if rc == 0:
            shape = (len(g["left_scalars"]), len(g["right_scalars"]))
            break
    assert shape is not None, "no proof has a Guard: give the shape"
    out = []
    for (rc, g), m in zip(raws, mult):
        if rc != 0:
            out.append(dict(left_scalars=[0] * shape[0], left_bases=[ZERO] * shape[0], right_scalars=[0] * shape[1], right_bases=[ZERO] * shape[1],
                            mult=m, status=rc))
            continue
        assert (len(g["left_scalars"]), len(g["right_scalars"])) == shape, "the term counts do not depend on the proof"
        out.append(dict(left_scalars=[s * m % R_MOD for s in g["left_scalars"]], left_bases=g["left_bases"],
                        right_scalars=[s * m % R_MOD for s in g["right_scalars"]], right_bases=g["right_bases"], mult=m, status=0))
    return out


def by_base(scalars, bases):
    """{base: sum of its scalars mod r}, zero sums and the identity left out: what two sum-equal term lists agree on"""
    acc = {}
    for s, b in zip(scalars, bases):
        acc[b] = (acc.get(b, 0) + s) % R_MOD
    return {b: s for b, s in acc.items() if s and b != ZERO}


# ---- the kernel's model

def gather(order, slot_scal, shared, pts, status, n, np_, first, count):
    """k_guards_gather over programmed arrays -> (scalars, bases) of the count * len(order) output terms.
    order: [(kind, index)]; slot_scal[p * np_ + slot], shared[j][p]: ints; pts[p * np_ + slot] and pts[n * np_ + j]: 64 bytes each;
    status[p]: the device's words."""
    scalars, bases = [], []
    for p in range(first, first + count):
        dead = decode_status(status[p]) != 0
        for kind, idx in order:
            if dead:
                scalars.append(0); bases.append(ZERO)
            elif kind:
                scalars.append(shared[idx][p]); bases.append(pts[n * np_ + idx])
            else:
                scalars.append(slot_scal[p * np_ + idx]); bases.append(pts[p * np_ + idx])
    return scalars, bases


def proofs_model(mult, status, first, count):
    """k_guards_proofs -> (multipliers, decoded statuses) of the range"""
    return list(mult[first:first + count]), [decode_status(s) for s in status[first:first + count]]
