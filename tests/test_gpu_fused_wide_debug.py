"""The wide small-minibatch loop (rr_svi_wide.hip) under the bounds-checking build of the library (`make debug`, -DRR_BOUNDS):
guard bands around every device allocation -- the per-(item, component) partial sums among them -- the kernels' assertions on
item bounds, child column ranges, row indices and length-scale slots, every launch checked for "current device == the stream's
device", and the launches COUNTED: n steps are n x (A, B, C, D), n candidates n x (A, B, D), nothing else of that file per step.
Three of the reference's fits, one oracle fit, the bitwise tests and the edges of tests/test_gpu_fused_wide.py run against it in
a subprocess, as tests/test_gpu_fused_svi_centres_debug.py runs the LDS kernel's."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

DEBUG_LIB = os.path.join(ROOT, "revrand_amd", "lib", "librevrand_hip_debug.so")
FILE = "tests/test_gpu_fused_wide.py::"
EDGES = ["K1_L5_M7", "K32_L3_M64", "K8_L20_M16", "bound_run_into", "child_boundary", "item_plus_one", "one_frequency",
         "one_minibatch_of_all_rows", "positive_upper"]
CASES = [FILE + "test_reference_fits_on_the_wide_loop[poisson_ard_bs10_ns5]",
         FILE + "test_reference_fits_on_the_wide_loop[gaussian_cat_bs10_ns5]",
         FILE + "test_reference_fits_on_the_wide_loop[binomial_cat_bs64f_ns0_momentum]",
         FILE + "test_wide_shape_against_the_oracle[gaussian]",
         FILE + "test_runs_and_blocks_of_steps_are_bit_identical",
         FILE + "test_chunked_random_starts_are_bit_identical",
         FILE + "test_launches_per_step_and_per_candidate"] + [FILE + "test_edges_against_the_host_loop[%s]" % e for e in EDGES]


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_bounds_build_runs_the_wide_loop():
    assert os.path.exists(DEBUG_LIB), "the entry point's build() makes librevrand_hip_debug.so (make -C revrand_amd/csrc debug)"
    env = dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + CASES + ["-m", "gpu"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=800)
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
    assert "%d passed" % len(CASES) in r.stdout, r.stdout[-500:]
