"""The one runner of the kernel unit harnesses (tests/cpp/*_units.hip, built by halo2_verifier_amd/csrc/Makefile): where a program
lies, one child process per call under a time limit, and the word and byte helpers of the file formats."""
import os
import struct
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def exe(name):
    path = os.path.join(ROOT, "halo2_verifier_amd", "csrc", "build", name)
    assert os.path.exists(path), path + " is missing: build() makes it (halo2_verifier_amd/csrc/Makefile)"
    return path


def start(name, args, timeout=120):
    """the program `name` once, in a fresh child process without standard input -> the finished process, whatever its status"""
    return subprocess.run([exe(name)] + [str(a) for a in args], capture_output=True, text=True, stdin=subprocess.DEVNULL, timeout=timeout)


def run(name, args, blob=None, tmp_path=None, timeout=120):
    """the program `name` once through start(): args are its operands, the output file last.  With a blob, the input and
    output files are made under tmp_path and their names follow args (the mode).  -> the output file's bytes"""
    args = [str(a) for a in args]
    if blob is not None:
        src, dst = tmp_path / (args[0] + "_in.bin"), tmp_path / (args[0] + "_out.bin")
        src.write_bytes(blob)
        args += [str(src), str(dst)]
    r = start(name, args, timeout)
    assert r.returncode == 0, (name, args[0], r.returncode, r.stderr[-2000:])
    with open(args[-1], "rb") as f:
        return f.read()


def words(seq):
    return np.asarray(seq, dtype="<u4").tobytes()


def as_words(raw):
    return np.frombuffer(raw, dtype="<u4")


class Cursor:
    """over a program's output bytes"""
    def __init__(self, raw): self.raw, self.at = raw, 0
    def take(self, n):
        assert self.at + n <= len(self.raw), "output too short"
        b = self.raw[self.at:self.at + n]; self.at += n; return b
    def word(self): return struct.unpack("<I", self.take(4))[0]
    def sword(self): return struct.unpack("<i", self.take(4))[0]
    def num(self): return int.from_bytes(self.take(32), "little")
    def done(self): assert self.at == len(self.raw), "output longer than its jobs"
