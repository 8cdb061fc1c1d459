"""The dimension-blocked centre kernels under the bounds-checking build of the library (`make debug`, -DRR_BOUNDS): guard
bands around every device allocation, the kernels' index assertions (the blocked indices of the wide feature kernels among
them), every launch checked for "current device == the stream's device" -- the ragged shapes, the one-live-dimension and
padding identities, the chunked second pass and the GLM loops of tests/test_gpu_centres_wide.py run against it in a
subprocess, as tests/test_gpu_centres_debug.py runs the narrow kernels'."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

DEBUG_LIB = os.path.join(ROOT, "revrand_amd", "lib", "librevrand_hip_debug.so")
CASES = ["tests/test_gpu_centres_wide.py::test_ragged_shapes_vs_restatement",
         "tests/test_gpu_centres_wide.py::test_ragged_shape_at_d_1000",
         "tests/test_gpu_centres_wide.py::test_one_live_dimension_equals_the_one_dimensional_basis",
         "tests/test_gpu_centres_wide.py::test_constant_columns_behind_128_change_no_bit",
         "tests/test_gpu_centres_wide.py::test_second_pass_chunked_and_bitwise_reproducible",
         "tests/test_gpu_centres_wide.py::test_second_pass_float64_chunked_and_bitwise_reproducible",
         "tests/test_gpu_centres_wide.py::test_one_live_dimension_contraction",
         "tests/test_gpu_centres_wide.py::test_glm_resident_loop_equals_the_default_host_loop",
         "tests/test_gpu_centres_wide.py::test_glm_group_resident_fit_equals_the_one_context_fit"]


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_bounds_build_runs_the_wide_centre_kernels():
    assert os.path.exists(DEBUG_LIB), "the entry point's build() makes librevrand_hip_debug.so (make -C revrand_amd/csrc debug)"
    env = dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + CASES + ["-m", "gpu"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
