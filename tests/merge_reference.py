"""Big-integer reference for the fold of a merge (k_accumulator_merge_fold, halo2_verifier_amd/csrc/util.hip), written from its
definition in csrc/internal.h over the affine G1 arithmetic of tests/msm_reference.py.  Nothing here ports the kernel: the sum is a
plain loop, whatever team the kernel runs with.

    acc[side] <- acc[side] + sum_k record_k[side]          record k's point of a side: piece 0 (records of whole points)
    sums[2 slot_k + side] <- record_k[side]                slot_k = slots[k], or k without a map; every other slot is left alone
"""
import msm_reference as ref

MERGE_MAX = 512             # include/h2v.h H2V_ACC_MERGE_MAX
STATE_BYTES = 152           # include/h2v.h H2V_ACC_STATE_BYTES
STATE_MAGIC = 0x53563248    # "H2VS"
STATE_VERSION = 1


def host_team(n):
    """the lanes per side the host picks for n records: min(64, the next power of two >= n + 1) (the previous accumulator is item 0)"""
    t = 1
    while t < 64 and t < n + 1:
        t *= 2
    return t


def dependent_additions(n, team):
    """the additions on lane 0's chain: its items, then one per butterfly level"""
    return -(-(n + 1) // team), team.bit_length() - 1


def merge_fold(acc, records, slots=None):
    """acc: (left, right) affine points (None: the identity); records: [(left, right)].
    -> ((left, right) after the fold, {slot: (left, right)} of the journal slots written)"""
    out = list(acc)
    for left, right in records:
        out[0], out[1] = ref.add(out[0], left), ref.add(out[1], right)
    written = {(slots[k] if slots is not None else k): rec for k, rec in enumerate(records)}
    assert len(written) == len(records)
    return tuple(out), written


def pack_state(left_xy, right_xy, n_proofs, n_failed, magic=STATE_MAGIC, version=STATE_VERSION):
    """the documented layout of an exported accumulator, composed byte by byte (include/h2v.h H2V_ACC_STATE_BYTES)"""
    assert len(left_xy) == 64 and len(right_xy) == 64
    out = magic.to_bytes(4, "little") + version.to_bytes(4, "little") + n_proofs.to_bytes(8, "little") + n_failed.to_bytes(8, "little") + left_xy + right_xy
    assert len(out) == STATE_BYTES
    return out
