"""The one builder and runner of the C++ caller programs (tests/cpp/*.cpp over tests/cpp/caller.h: stand-alone programs that drive the
library as a user would, through include/h2v.hpp, include/h2v_guards.hpp and the C ABI), the sibling of units_harness.py: one set of
compiler flags, the writers of the files a program reads (their formats are documented at the top of tests/cpp/caller.h), one child
process per run under a time limit, and the helpers that read what a program or a stand-in library printed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
FLAGS = ["-std=c++17", "-O1", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include")]
# (the sanitizers' runtimes linked statically: the program then starts whatever else the environment preloads)
SANITIZE = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-static-libubsan"]


def _compile(cmd):
    r = subprocess.run(cmd, capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=600)
    assert r.returncode == 0, (" ".join(cmd), r.stderr[-2000:])


def build(name, tmp_path, hip=False, sanitize=False, stubs=(), defines=(), shared=False):
    """tests/cpp/<name>.cpp into tmp_path -> the program's path.  It is linked with the stand-in libraries named in `stubs`
    (tests/cpp/<stub>.cpp) or, without any, with the built library; hip: host code over the HIP runtime's API, built by hipcc for its
    include and library paths, in two steps so that only the source is read as HIP; sanitize: under the address and undefined-behaviour
    sanitizers; shared: a shared library of the source alone (a stand-in that ctypes loads)."""
    flags = FLAGS + ["-D" + d for d in defines] + (SANITIZE if sanitize else [])
    src = os.path.join(CPP, name + ".cpp")
    if shared:
        out = tmp_path / ("lib" + name + ".so")
        _compile(["g++"] + flags + ["-shared", "-fPIC", "-o", str(out), src])
        return out
    out = tmp_path / name
    if stubs:
        link = [os.path.join(CPP, s + ".cpp") for s in stubs]
    else:
        from halo2_verifier_amd import _lib
        link = [_lib.lib_path(), "-Wl,-rpath," + os.path.dirname(_lib.lib_path())]
    if hip:
        obj = tmp_path / (name + ".o")
        _compile(["hipcc"] + flags + ["--offload-arch=gfx950", "-c", "-o", str(obj), src])
        _compile(["hipcc", "-o", str(out), str(obj)] + link)
    else:
        _compile(["g++"] + flags + ["-o", str(out), src] + link)
    return out


def check_syntax(src):
    """a source file (a name under tests/cpp, or a path) is valid C++17 against the headers of include/, warnings as errors"""
    _compile(["g++"] + FLAGS + ["-fsyntax-only", os.path.join(CPP, str(src))])


def run(exe, args=(), timeout=300, allow_fail=False, env=None):
    """the program once, in a fresh child process without standard input -> the finished process; a status other than zero fails the
    test with the end of the program's stderr, unless the test expects one (allow_fail)"""
    r = subprocess.run([str(exe)] + [str(a) for a in args], capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=timeout, env=env)
    assert allow_fail or r.returncode == 0, (os.path.basename(str(exe)), r.returncode, r.stderr[-2000:])
    return r


def lines(out, prefix):
    """the lines of a program's output (a string, or its lines) that start with prefix (a string or a tuple of them)"""
    return [l for l in (out.splitlines() if isinstance(out, str) else out) if l.startswith(prefix)]


def fnv(b):
    """length:hash as the stand-in libraries print an array they were handed (tests/cpp/h2v_stub.h)"""
    h = 1469598103934665603
    for x in b:
        h = ((h ^ x) * 1099511628211) & 0xffffffffffffffff
    return "%d:%016x" % (len(b), h)


def hex_word(b):
    return b.hex() or "-"


def items_text(P, I, keys=None, header=None):
    """items.txt for the proofs P with the instances I (per proof its columns, each a list of 32-byte values): keyed, under "n_keys n",
    when keys gives every proof's key, unkeyed under "n" otherwise; a header of the caller's own replaces either"""
    if header is None:
        header = "%d %d" % (max(keys, default=0) + 1, len(P)) if keys is not None else "%d" % len(P)
    out = [header]
    for i, (p, inst) in enumerate(zip(P, I)):
        words = [str(keys[i])] if keys is not None else []
        words += [str(len(inst))] + [str(len(c)) for c in inst] + [hex_word(p), hex_word(b"".join(v for col in inst for v in col))]
        out.append(" ".join(words))
    return "\n".join(out) + "\n"


def keyed_items_text(items, setups):
    """the keyed items.txt for (setup, proof, instances) triples: a proof's key is the place of its setup in setups"""
    return items_text([p for _, p, _ in items], [i for _, _, i in items], keys=[[s is t for t in setups].index(True) for s, _, _ in items],
                      header="%d %d" % (len(setups), len(items)))


def stand_in_items_text(n):
    """the keyed items.txt of n made-up proofs of one key for a run over a stand-in library: 40 bytes each, two columns of one value"""
    return items_text([bytes([i]) * 40 for i in range(n)], [[[b"\xab" * 32], [b"\xab" * 32]]] * n, keys=[0] * n)


def guards_text(guards):
    """guards.txt for Guards given as dicts of lists (left_scalars, left_bases, right_scalars, right_bases)"""
    return "".join(" ".join(hex_word(b"".join(g[k])) for k in ("left_scalars", "left_bases", "right_scalars", "right_bases")) + "\n" for g in guards)


def draws(rand):
    """ints or 32-byte strings -> the bytes of rand.bin"""
    return rand if isinstance(rand, bytes) else b"".join(r if isinstance(r, bytes) else r.to_bytes(32, "little") for r in rand)


def write_dir(d, params=None, vk=None, vks=(), rand=None, **files):
    """the directory a program is given: params.bin, vk.bin (vk) or vk<k>.bin (vks), rand.bin, and further files by name with dots as
    underscores (items_txt=..., seed_bin=...): bytes, or text"""
    files = {name[::-1].replace("_", ".", 1)[::-1]: data for name, data in files.items()}
    if params is not None:
        files["params.bin"] = params
    if vk is not None:
        files["vk.bin"] = vk
    for k, key in enumerate(vks):
        files["vk%d.bin" % k] = key
    if rand is not None:
        files["rand.bin"] = draws(rand)
    for name, data in files.items():
        if isinstance(data, str):
            (d / name).write_text(data)
        else:
            (d / name).write_bytes(data)
    return d
