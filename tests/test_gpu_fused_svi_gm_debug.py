"""The fused small-minibatch kernel's spectral-mixture children under the bounds-checking build of the library (`make debug`,
-DRR_BOUNDS): guard bands around every device allocation -- the per-component scalars `pubsc`, widened by 2 Xdim slots per
component, among them -- and the kernel's index assertions where it reads V in LDS, the [mean | length scales] slots, the row
phases parked in Q and the four column blocks.  The three oracle checks and the Xdim = 3 fit of
tests/test_gpu_fused_svi_gm.py run against it in a subprocess, as tests/test_gpu_fused_svi_centres_debug.py runs the centre
children."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

DEBUG_LIB = os.path.join(ROOT, "revrand_amd", "lib", "librevrand_hip_debug.so")
FILE = "tests/test_gpu_fused_svi_gm.py::"
CASES = [FILE + "test_mixed_children_one_step_against_the_oracle",
         FILE + "test_mixed_children_four_adam_steps_with_the_log_trick",
         FILE + "test_mixed_children_random_starts_against_the_oracle",
         FILE + "test_a_spectral_mixture_on_three_columns_runs_on_both_device_loops"]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bounds_build_runs_the_fused_kernel_s_spectral_mixture_children():
    assert os.path.exists(DEBUG_LIB), "the entry point's build() makes librevrand_hip_debug.so (make -C revrand_amd/csrc debug)"
    env = dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + CASES + ["-m", "gpu"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
    assert "4 passed" in r.stdout, r.stdout[-500:]
