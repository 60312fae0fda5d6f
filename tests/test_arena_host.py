"""CPU: the workspace carver (python-world_amd/csrc/wh_arena.h) as a stand-alone host program, tests/arena_check.cpp —
byte-identical offsets to the hand-written layouts it replaced, optional and failed regions, and every region's first and
last element written in a real allocation, under AddressSanitizer and UBSan where the host compiler links them."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def _compiler():
    for cxx in ("c++", "/opt/rocm/llvm/bin/clang++"):
        path = shutil.which(cxx)
        if path:
            return path
    pytest.fail("no host C++ compiler (c++ or /opt/rocm/llvm/bin/clang++)")


def test_carver_matches_the_hand_written_layouts(tmp_path):
    cxx = _compiler()
    exe = str(tmp_path / "arena_check")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I", os.path.join(ROOT, "python-world_amd", "csrc"),
            os.path.join(HERE, "arena_check.cpp"), "-o", exe]
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # The sanitizer runtime linked into the program where the compiler can (GCC's is a shared library by default, and that
    # one refuses to start in a process whose environment preloads any other library), else as the compiler links it,
    # else none: the program's own assertions stand on their own.
    run = None
    for extra in (san + ["-static-libasan", "-static-libubsan"], san, []):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=120)
        if r.returncode != 0:
            assert extra, r.stderr[-3000:]
            continue
        run = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        if extra and "ASan runtime does not come first" in run.stderr:
            continue
        print("built with", extra or "no sanitizer")
        break
    assert run.returncode == 0, (run.stdout[-3000:], run.stderr[-3000:])
    assert run.stdout.strip().endswith("arena_check: ok")
