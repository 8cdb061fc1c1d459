"""The FastFood children of the float64 feature matrix under the bounds-checking build of the library (`make debug`,
-DRR_BOUNDS): guard bands around every device allocation, the extent assertions of the chain kernels, of rr_fm64_form_a_kernel /
rr_fm64_stage_x_kernel / rr_fm64_xt_sum_kernel and of the row-slab form of rr_gemm_tn_f64_kernel -- the put, contraction and
ragged-concatenation cases of tests/test_gpu_fastfood_f64.py run against it in a subprocess."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

DEBUG_LIB = os.path.join(ROOT, "revrand_amd", "lib", "librevrand_hip_debug.so")
CASES = ["tests/test_gpu_fastfood_f64.py::test_put_fastfood_writes_float64_features_and_nothing_else",
         "tests/test_gpu_fastfood_f64.py::test_put_fastfood_gm_writes_float64_features_and_nothing_else",
         "tests/test_gpu_fastfood_f64.py::test_put_fastfood_gm_against_the_recorded_reference_on_a_wide_handle",
         "tests/test_gpu_fastfood_f64.py::test_the_contraction_is_exact",
         "tests/test_gpu_fastfood_f64.py::test_the_wide_contraction_repeats_bit_for_bit_on_real_data",
         "tests/test_gpu_fastfood_f64.py::test_glm_step_with_fastfood_children_vs_oracle",
         "tests/test_gpu_fastfood_f64.py::test_glm_resident_gather_equals_host_rows_bit_for_bit"]


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_bounds_build_runs_the_float64_fastfood_children():
    assert os.path.exists(DEBUG_LIB), "the entry point's build() makes librevrand_hip_debug.so (make -C revrand_amd/csrc debug)"
    env = dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + CASES + ["-m", "gpu"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]
