"""The float64 GLM step under the bounds-checking build of the library (`make debug`, -DRR_BOUNDS): guard bands around every
device allocation, the extent assertions in the step's kernels and in the row-slab form of rr_gemm_tn_f64_kernel, and every
launch checked for "current device == the stream's device" -- the golden step, the ragged concatenations, the tile-edge /
row-slab test and the resident gather of tests/test_gpu_glm_f64.py run against it in a subprocess."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

DEBUG_LIB = os.path.join(ROOT, "revrand_amd", "lib", "librevrand_hip_debug.so")
CASES = ["tests/test_gpu_glm_f64.py::test_minibatch_elbo_vs_reference",
         "tests/test_gpu_glm_f64.py::test_ragged_concatenation_vs_oracle",
         "tests/test_gpu_glm_f64.py::test_every_tile_edge_and_the_row_slabs",
         "tests/test_gpu_glm_f64.py::test_resident_gather_equals_host_rows_bit_for_bit"]


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_bounds_build_runs_the_float64_glm_step():
    assert os.path.exists(DEBUG_LIB), "the entry point's build() makes librevrand_hip_debug.so (make -C revrand_amd/csrc debug)"
    env = dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + CASES + ["-m", "gpu"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
