"""GroupShape (halo2_verifier_amd/csrc/batch.h), the description of a batch's groups that the host code and the kernels share, run on
the HOST against brute force over every proof and draw index: first, count, of, draw_at, zero_below, largest and fits, for equal and
unequal groups (tests/cpp/group_shape_host.hip).  The program is compiled with its host side under the address and undefined-behaviour
sanitizers and run directly.  No GPU needed."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_shape_matches_brute_force_under_sanitizers(tmp_path):
    exe = tmp_path / "group_shape_host"
    src = os.path.join(ROOT, "tests", "cpp", "group_shape_host.hip")
    r = subprocess.run(["hipcc", "-O1", "-g", "-std=c++17", "--offload-arch=gfx950", "-Xarch_host", "-fsanitize=address,undefined",
                        "-Xarch_host", "-fno-sanitize-recover=all", "-o", str(exe), src], capture_output=True, text=True)
    assert r.returncode == 0, "hipcc failed: " + r.stderr[-2000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = r.stdout.split("\n")
    assert lines[-2:] == ["ok", ""] and not r.stderr
    # 2 x 2 x 2 equal shapes and the three unequal ones were walked
    assert len([l for l in lines if l.startswith("equal: ")]) == 8 and len([l for l in lines if l.startswith("unequal: ")]) == 3
