"""The mixture mode of the wide FastFood chain kernel under the bounds-checking build of the library (`make debug`,
-DRR_BOUNDS): guard bands around every device allocation, the kernel's extent (4 n <= ldo) and permutation-entry assertions,
every launch checked for "current device == the stream's device" -- the grid, variant, dtype, rows-per-workgroup and
feature-matrix cases of tests/test_gpu_fastfood_gm_wide.py run against it once in a subprocess, as
tests/test_gpu_fastfood_wide_debug.py runs the wide kernel's other modes.  A second subprocess takes the census: under the
counting library each case ran the `.../gm/...` instance the table in tests/fastfood_gm_wide_cases.py names, once, and no other
instance of the wide or the narrow families."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

DEBUG_LIB = os.path.join(ROOT, "revrand_amd", "lib", "librevrand_hip_debug.so")
CASES = ["tests/test_gpu_fastfood_gm_wide.py::test_every_instance_is_exact",
         "tests/test_gpu_fastfood_gm_wide.py::test_variants_and_untouched_elements",
         "tests/test_gpu_fastfood_gm_wide.py::test_every_dtype_combination_is_exact",
         "tests/test_gpu_fastfood_gm_wide.py::test_rows_per_workgroup_seam",
         "tests/test_gpu_fastfood_gm_wide.py::test_feature_matrix_block_and_untouched_columns"]


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_bounds_build_runs_the_wide_mixture_mode():
    assert os.path.exists(DEBUG_LIB), "the entry point's build() makes librevrand_hip_debug.so (make -C revrand_amd/csrc debug)"
    env = dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB)
    r = subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + CASES + ["-m", "gpu"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=1500)
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])
    assert " passed" in r.stdout and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_each_case_runs_the_instance_the_table_names():
    assert os.path.exists(DEBUG_LIB), "the entry point's build() makes librevrand_hip_debug.so (make -C revrand_amd/csrc debug)"
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\nimport fastfood_gm_wide_cases as gc\n"
            "for label, got, want in gc.census():\n    print('CENSUS', label, want, sorted(got.items()))\n"
            % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB), capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])
    import fastfood_gm_wide_cases as gc
    lines = [ln.split(" ", 3) for ln in r.stdout.splitlines() if ln.startswith("CENSUS ")]
    assert len(lines) == len(gc.census_runs())
    seen = set()
    for _, label, want, got in lines:
        assert got == repr([(want, 1)]), (label, want, got)
        seen.add(want)
    assert seen == set(gc.all_idents())
