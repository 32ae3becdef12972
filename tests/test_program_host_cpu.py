"""The host unit of the executor (csrc/yl_program.cpp: validation, weight packing, derived tables) under AddressSanitizer
and UndefinedBehaviorSanitizer: tests/host/program_host.cpp, a stand-alone program, is compiled together with the unit by
ROCm's host clang and run.  It is linked against the built library for the four shape predicates only; nothing is loaded
into this process."""
import os
import subprocess

import pytest

from yololite_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "yololite-official-repo_amd", "csrc")


def _clang():
    for c in (os.environ.get("YL_HOST_CXX"), "/opt/rocm/lib/llvm/bin/clang++", "/opt/rocm/llvm/bin/clang++"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("ROCm's host clang++ not found")


def test_validate_and_pack_are_memory_clean(tmp_path):
    lib = os.path.abspath(_lib.LIB_PATH)
    exe = str(tmp_path / "program_host")
    cmd = [_clang(), "-std=c++17", "-O1", "-g", "-fno-omit-frame-pointer", "-fsanitize=address,undefined",
           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tests", "host", "program_host.cpp"),
           os.path.join(CSRC, "yl_program.cpp"), lib, "-Wl,-rpath," + os.path.dirname(lib), "-o", exe]
    built = subprocess.run(cmd, capture_output=True, text=True)
    assert built.returncode == 0, built.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and run.stdout.strip().endswith("ok"), (run.stdout[-2000:], run.stderr[-4000:])
