"""The fused small-minibatch kernel's centre and polynomial children under the bounds-checking build of the library (`make
debug`, -DRR_BOUNDS): guard bands around every device allocation -- the published columns and the widened per-component
scalars (`pubsc`: one slot per length scale of every random Fourier AND centre child, plus four) among them -- the kernel's
index assertions where it reads the centre table in LDS and the length-scale slots, every launch checked for "current
device == the stream's device".  T1, T2 and three of T3's fits of tests/test_gpu_fused_svi_centres.py (radial ARD, sigmoid
isotropic, the concatenation) run against it in a subprocess, as tests/test_gpu_centres_wide_debug.py runs the wide kernels."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

DEBUG_LIB = os.path.join(ROOT, "revrand_amd", "lib", "librevrand_hip_debug.so")
FILE = "tests/test_gpu_fused_svi_centres.py::"
CASES = [FILE + "test_one_step_against_the_reference_s_gradient",
         FILE + "test_mixed_children_one_step_against_the_oracle",
         FILE + "test_mixed_children_four_adam_steps_with_the_log_trick",
         FILE + "test_mixed_children_random_starts_against_the_oracle",
         FILE + "test_centre_children_fused_equals_the_other_two[radial_ard-poisson-4]",
         FILE + "test_centre_children_fused_equals_the_other_two[sigmoid_iso-poisson-1]",
         FILE + "test_concatenation_with_an_rff_and_two_centre_children"]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bounds_build_runs_the_fused_kernel_s_centre_and_polynomial_children():
    assert os.path.exists(DEBUG_LIB), "the entry point's build() makes librevrand_hip_debug.so (make -C revrand_amd/csrc debug)"
    env = dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + CASES + ["-m", "gpu"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
    assert "7 passed" in r.stdout, r.stdout[-500:]
