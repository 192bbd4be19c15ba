"""What a finish into device memory (h2v_batch_finish_device: k_results_tiles, k_results_close, k_results_scatter,
halo2_verifier_amd/csrc/util.hip) must leave, in Python integers and lists: the decoded statuses, every group's count of failing
proofs for equal and unequal groups, group_ok, the failing proofs' indices in ascending order under a cap, and the summary words —
finish_impl's rules (csrc/batch.hip) restated.  tests/test_results_reference.py holds it against hand-written cases."""

# the device's rank codes (csrc/batch.h) -> the ABI's codes (include/h2v.h); every other word passes through
DECODE = {0: 0, -40: -1, -30: -5, -20: -7, -10: -4}
NO_FAULT = 0xffffffff
SUMMARY_WORDS = 8
FLAG_PAIRING, FLAG_FOLDED = 1, 2


def decode(word: int) -> int:
    return DECODE.get(word, word)


def offsets(n, groups=1, sizes=None):
    """where the groups lie: `sizes`, or `groups` equal slices of n proofs"""
    if sizes is None:
        assert groups >= 1 and n % groups == 0
        sizes = [n // groups] * groups
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    assert off[-1] == n
    return off


def group_failed(words, groups=1, sizes=None):
    """per group: its proofs whose status word is not 0"""
    off = offsets(len(words), groups, sizes)
    return [sum(1 for w in words[off[g]:off[g + 1]] if w != 0) for g in range(len(off) - 1)]


def group_ok(failed, fold_failed, ok, pairing, fault=NO_FAULT):
    """finish_impl's verdict: no failing proof, no failed proof reported by a fold, and — only if the launch ran its own pairing —
    the pairing's word; a draw fault rejects every group"""
    return [1 if (f == 0 and ff == 0 and (not pairing or o != 0) and fault == NO_FAULT) else 0 for f, ff, o in zip(failed, fold_failed, ok)]


def failed_index(words, cap=None):
    """the proofs whose status word is not 0, ascending; the first `cap` of them"""
    idx = [i for i, w in enumerate(words) if w != 0]
    return idx if cap is None else idx[:cap]


def split_xy(out_bytes: bytes, groups: int):
    """the results block's 128 bytes per group -> (left, right), 64 bytes per group each"""
    assert len(out_bytes) == 128 * groups
    left = b"".join(out_bytes[128 * g:128 * g + 64] for g in range(groups))
    right = b"".join(out_bytes[128 * g + 64:128 * g + 128] for g in range(groups))
    return left, right


def summary(words, oks, groups, flags, fault=NO_FAULT):
    return [fault, sum(1 for w in words if w != 0), sum(oks), len(words), groups, flags, 0, 0]


def finish(words, fold_failed, ok, out_bytes, flags, groups=1, sizes=None, fault=NO_FAULT, cap=None):
    """everything at once -> dict of the seven outputs"""
    G = len(sizes) if sizes is not None else groups
    failed = group_failed(words, groups, sizes)
    oks = group_ok(failed, fold_failed, ok, bool(flags & FLAG_PAIRING), fault)
    left, right = split_xy(out_bytes, G)
    return {"status": [decode(w) for w in words], "group_ok": oks, "left_xy": left, "right_xy": right, "group_failed": failed,
            "failed_index": failed_index(words, cap), "summary": summary(words, oks, G, flags, fault)}
