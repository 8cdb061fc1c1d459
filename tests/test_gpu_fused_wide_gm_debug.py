"""Spectral-mixture items of the wide small-minibatch loop (rr_svi_wide.hip) under the bounds-checking build of the library
(`make debug`, -DRR_BOUNDS): guard bands around every device allocation, the kernels' assertions on the GM item bounds
(j0 + cnt <= n, width == 4 n, slot ranges < maxls), every launch checked and COUNTED.  The oracle tests, the bitwise tests, the
routing of the report's shape and the launch counts of tests/test_gpu_fused_wide_gm.py run against it in a subprocess, as
tests/test_gpu_fused_wide_debug.py runs the loop's other children.  (Not a sanitizer run.)"""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

DEBUG_LIB = os.path.join(ROOT, "revrand_amd", "lib", "librevrand_hip_debug.so")
FILE = "tests/test_gpu_fused_wide_gm.py::"
CASES = [FILE + "test_mixed_children_one_step_against_the_oracle[3]",
         FILE + "test_mixed_children_one_step_against_the_oracle[None]",
         FILE + "test_mixed_children_four_adam_steps_with_the_log_trick",
         FILE + "test_one_component_on_128_columns_fills_every_slot[2]",
         FILE + "test_one_component_on_128_columns_fills_every_slot[1]",
         FILE + "test_reruns_and_cuts_into_calls_are_bit_identical",
         FILE + "test_blocks_of_steps_and_chunks_of_starts_are_bit_identical_through_the_model",
         FILE + "test_four_components_take_the_wide_loop",
         FILE + "test_launches_per_step_and_per_candidate"]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bounds_build_runs_the_spectral_mixture_items():
    assert os.path.exists(DEBUG_LIB), "the entry point's build() makes librevrand_hip_debug.so (make -C revrand_amd/csrc debug)"
    env = dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + CASES + ["-m", "gpu"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
    assert "%d passed" % len(CASES) in r.stdout, r.stderr[-500:] + r.stdout[-500:]
