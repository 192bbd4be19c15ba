"""The batch multipliers of groups of unequal size in Python integers: mult[p] = the product, mod r, of the draws of the LATER proofs of
p's own group (kzg/strategy.rs:129, msm.rs:173-176, per group).  Two forms: the definition, group by group, and the segmented suffix
scan the kernels run (csrc/verify_kernels.hip: k_seg_mult_tiles / k_seg_mult_scan_tiles / k_seg_mult_apply) with its (value, closed)
pairs, tiles and chunks — so that a failure of the kernels can be told from a failure of the scheme."""

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
MULT_TILE = 256       # draws per tile (verify_kernels.hip)
SCAN_CHUNK = 1024     # tile products per round of the scan over tiles


def offsets(sizes):
    off = [0]
    for s in sizes:
        assert s >= 1
        off.append(off[-1] + s)
    return off


def last_flags(sizes):
    """per proof: it is the last of its group (what the host copies beside the draws)"""
    flags = [0] * sum(sizes)
    for end in offsets(sizes)[1:]:
        flags[end - 1] = 1
    return flags


def multipliers(sizes, draws):
    """the definition: every group on its own"""
    assert len(draws) == sum(sizes)
    out, off = [0] * len(draws), offsets(sizes)
    for g in range(len(sizes)):
        run = 1
        for j in range(off[g + 1] - 1, off[g] - 1, -1):
            out[j] = run
            run = run * draws[j] % R
    return out


def combine(a, b):
    """the pair of two adjacent spans of draws, a in front of b: (v, closed) = (the product from the span's first draw to the end of
    that draw's group or of the span, whether the group ends inside the span)"""
    return a if a[1] else (a[0] * b[0] % R, b[1])


def _suffix_scan(pairs):
    """Hillis-Steele over one workgroup's pairs: part[t] <- the pair of the span [t, T)"""
    part, T, d = list(pairs), len(pairs), 1
    while d < T:
        part = [combine(part[t], part[t + d] if t + d < T else (1, 0)) for t in range(T)]
        d <<= 1
    return part


def multipliers_scan(sizes, draws, tile=MULT_TILE, chunk=SCAN_CHUNK):
    """the kernels' scheme"""
    n, last = len(draws), last_flags(sizes)
    tiles = (n + tile - 1) // tile
    mult, tile_pair, open_from = [0] * n, [], []
    for b in range(tiles):
        pairs = [(draws[j], last[j]) if j < n else (1, 1) for j in range(b * tile, (b + 1) * tile)]
        part = _suffix_scan(pairs)
        for t in range(tile):
            j = b * tile + t
            if j < n:
                mult[j] = 1 if (pairs[t][1] or t + 1 == tile) else part[t + 1][0]
        closed = [p[1] for p in part]
        assert closed == sorted(closed, reverse=True)      # the closed spans are a prefix of the tile
        open_from.append(closed.index(0) if 0 in closed else tile)
        tile_pair.append(part[0])
    later, carry, hi = [1] * tiles, 1, tiles
    while hi > 0:
        lo = max(hi - chunk, 0)
        part = _suffix_scan([tile_pair[i] if i < hi else (1, 0) for i in range(lo, lo + chunk)])
        for t in range(hi - lo):
            nxt = part[t + 1] if t + 1 < chunk else (1, 0)
            later[lo + t] = nxt[0] if nxt[1] else nxt[0] * carry % R
        carry = part[0][0] if part[0][1] else part[0][0] * carry % R
        hi = lo
    for j in range(n):
        if j % tile >= open_from[j // tile]:
            mult[j] = mult[j] * later[j // tile] % R
    return mult


def tile_edge_sizes(n=1024, tile=MULT_TILE):
    """group sizes over n draws whose boundaries fall on every tile edge, and next to each"""
    cuts = sorted({c for e in range(tile, n, tile) for c in (e - 1, e, e + 1)} | {n})
    return [b - a for a, b in zip([0] + cuts, cuts)]
