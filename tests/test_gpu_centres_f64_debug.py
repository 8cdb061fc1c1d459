"""The float64 centre and polynomial kernels under the bounds-checking build of the library (`make debug`, -DRR_BOUNDS): guard
bands around every device allocation, the store-alignment and column-extent assertions in the kernels, and every launch checked
for "current device == the stream's device" -- the ragged feature blocks, the chunked contraction, the C ABI flow and the golden
`_elbo` cases of tests/test_gpu_centres_f64.py run against it in a subprocess."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

DEBUG_LIB = os.path.join(ROOT, "revrand_amd", "lib", "librevrand_hip_debug.so")
CASES = ["tests/test_gpu_centres_f64.py::test_feature_blocks_ragged_neighbours_intact",
         "tests/test_gpu_centres_f64.py::test_polynomial_features_in_the_float64_matrix",
         "tests/test_gpu_centres_f64.py::test_second_pass_chunked_and_bitwise_reproducible",
         "tests/test_gpu_centres_f64.py::test_device_rows_and_length_scales_recorded_by_the_put",
         "tests/test_gpu_centres_f64.py::test_elbo_f64_resident_vs_reference"]


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_bounds_build_runs_the_float64_centre_kernels():
    assert os.path.exists(DEBUG_LIB), "the entry point's build() makes librevrand_hip_debug.so (make -C revrand_amd/csrc debug)"
    env = dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + CASES + ["-m", "gpu"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
