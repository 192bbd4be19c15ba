"""What the two launches of an upload from device memory (h2v_batch_upload_device: k_ingest_rows, k_ingest_draws,
halo2_verifier_amd/csrc/util.hip) must leave, in Python integers and bytes: the packed rows, the stored draws, the fault word and
every group's zero_below — the last by the host rule of an upload from host memory (zero_below_of_draws, csrc/batch.hip), restated
loop for loop.  tests/test_ingest_reference.py holds it against a direct definition."""

R = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
NO_FAULT = 0xffffffff


def pack_rows(src: bytes, n: int, row_len: int, stride: int) -> bytes:
    """row i = src[i * stride : i * stride + row_len], one behind the other"""
    assert stride >= row_len and len(src) >= (n - 1) * stride + row_len if n else True
    return b"".join(src[i * stride:i * stride + row_len] for i in range(n))


def offsets(sizes):
    off = [0]
    for s in sizes:
        off.append(off[-1] + s)
    return off


def zero_below(draws, n, groups=1, sizes=None):
    """per group: the proofs [0, zero_below[g]) of the group have a zero draw behind them.  draws: integers, the uploaded tail.
    sizes: groups of unequal size (one draw per proof); else `groups` equal groups of n / groups proofs and len(draws) / groups draws."""
    if sizes is not None:
        off = offsets(sizes)
        assert len(draws) == n == off[-1]
        out = [0] * len(sizes)
        for g in range(len(sizes)):
            f, j = off[g], off[g + 1] - off[g]
            while j > 1:
                j -= 1
                if draws[f + j] == 0:
                    out[g] = j
                    break
        return out
    out = [0] * groups
    if n:
        assert n % groups == 0 and len(draws) % groups == 0 and len(draws) >= n
        gs, nt = n // groups, len(draws) // groups
        for g in range(groups):
            j = nt
            while j > 1:
                j -= 1
                if draws[g * nt + j] == 0:
                    out[g] = min(j, gs)
                    break
    return out


def ingest_draws(draws, n, groups=1, sizes=None):
    """-> (stored draws, fault word, zero_below): a draw >= r is stored as 1 and the lowest index of one is the fault word"""
    bad = [i for i, d in enumerate(draws) if d >= R]
    stored = [1 if d >= R else d for d in draws]
    return stored, (bad[0] if bad else NO_FAULT), zero_below(draws, n, groups, sizes)
