"""The library's host worker pool (revrand_amd/csrc/rr_workers.h) without a GPU.

tests/workers_stress.cpp, the header alone under the host compiler, holds the pool to its invariant -- every id in [0, n)
runs a job exactly once, no other id does, nothing runs after wait() -- through growth and shrink (the sequence of worker
counts 2, 2, 4, 4, 8, 3, 16, 1 on fresh pools, which the two classes this pool replaced failed: they ran a job on more
workers than it was started for), a caller that feeds the workers (rr_legacy_randn), a caller that takes part (the group
step), concurrent callers and a fork.  Built and run directly under ThreadSanitizer (without the fork: that runtime refuses
new threads after a multithreaded fork) and under AddressSanitizer with UBSan.
"""
import os
import shutil
import subprocess

import pytest

from conftest import ROOT

BUILDS = {"thread": (["-fsanitize=thread"], ["--no-fork"]),
          "address,undefined": (["-fsanitize=address,undefined", "-fno-sanitize-recover=all"], [])}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_workers_stress_under_sanitizers(tmp_path, build):
    """Exit status 0, the program's closing line (no failures; the fork scenario ran where it can), no sanitizer report."""
    cxx = shutil.which(os.environ.get("CXX", "g++")) or shutil.which("clang++")
    if build == "thread":
        # ROCm's clang++ as the host compiler where it is installed: its ThreadSanitizer runtime also starts on kernels that
        # randomise mappings over 32 bits, where GCC 11's gives up before main ("unexpected memory mapping")
        rocm = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin", "clang++")
        cxx = rocm if os.path.exists(rocm) else cxx
    assert cxx, "no host C++ compiler"
    flags, args = BUILDS[build]
    exe = str(tmp_path / "workers_stress")
    cmd = [cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-pthread"] + flags + [
        "-I", os.path.join(ROOT, "revrand_amd", "csrc"), os.path.join(ROOT, "tests", "workers_stress.cpp"), "-o", exe]
    c = subprocess.run(cmd, capture_output=True, text=True, timeout=300)
    assert c.returncode == 0, c.stderr[-3000:]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    last = r.stdout.strip().splitlines()[-1]
    assert " jobs hold, 0 failures" in last and ("fork skipped" in last) == bool(args), r.stdout[-500:]
    assert "FAILED" not in r.stdout and "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-3000:])
