"""The two entry points of include/h2v_draws.h are context-free: two host threads, each with its own stream and its own seed, make
interleaved expand_tensor calls (and host expansions between them), and every result is the definition's.  This test stands in for
the scene that tests/thread_scenes.py, whose table covers include/h2v.h, does not name."""
import hashlib
import threading

import pytest

pytestmark = pytest.mark.gpu

R_MOD = 0x30644e72e131a029b85045b68181585d2833e84879b9709143e1f593f0000001
CALLS = 50


def ref_expand(seed, first, n):
    return b"".join((int.from_bytes(hashlib.blake2b(seed + (first + j).to_bytes(8, "little"), digest_size=64, person=b"h2v-draws-v1").digest(), "little") % R_MOD)
                    .to_bytes(32, "little") for j in range(n))


def _plan(t):
    """thread t's calls: (first, n) with sizes spread over 1 .. 300, the two threads' sizes in opposite order"""
    sizes = [1 + (k * 299) // (CALLS - 1) for k in range(CALLS)]
    if t:
        sizes.reverse()
    return [((2**32 - 40 if k % 5 == 0 else 1000 * t) + 7 * k, n) for k, n in enumerate(sizes)]


def test_two_threads_two_streams_two_seeds():
    import torch
    import halo2_verifier_amd as h2v
    seeds = [bytes((17 * i + 3 + 101 * t) % 256 for i in range(32)) for t in range(2)]
    want = [[ref_expand(seeds[t], first, n) for first, n in _plan(t)] for t in range(2)]      # before the threads start
    torch.cuda.init()
    h2v.expand_tensor(seeds[0], 0, 1, 0)                 # (the library and the kernel are loaded)
    torch.cuda.synchronize()
    streams = [torch.cuda.Stream(device="cuda:0") for _ in range(2)]
    gate = threading.Barrier(2)
    results, errors = [None, None], []

    def work(t):
        try:
            torch.cuda.set_device(0)
            out, host = [], []
            gate.wait(timeout=60)
            for k, (first, n) in enumerate(_plan(t)):
                out.append(h2v.expand_tensor(seeds[t], first, n, 0, stream=streams[t]))
                if k % 10 == 0:
                    host.append((k, h2v.expand(seeds[t], first, n)))
            streams[t].synchronize()
            results[t] = ([bytes(x.cpu().numpy().tobytes()) for x in out], host)
        except Exception as e:       # (reported by the main thread)
            errors.append((t, repr(e)))

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads: th.start()
    for th in threads: th.join(120)
    assert not errors, errors
    assert all(not th.is_alive() for th in threads)
    for t in range(2):
        got, host = results[t]
        assert len(got) == CALLS and sorted({len(g) // 32 for g in got})[0] == 1 and max(len(g) // 32 for g in got) == 300
        assert got == want[t]
        assert all(h == want[t][k] for k, h in host)
