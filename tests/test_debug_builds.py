"""The sanitizer / bounds-checking builds of the library (`make asan`, `make debug`), when they are built:
* librevrand_hip_asan.so  -- host side of the C ABI under AddressSanitizer: the ABI checks (CPU) and the ragged-shape
  parity tests (GPU) run against it in a subprocess with the ASan runtime preloaded;
* librevrand_hip_debug.so -- -DRR_BOUNDS: guard bands around every device allocation + index assertions in the feature,
  SYRK, feature-matrix and FastFood kernels; the ragged-shape tests run against it on the GPU, and a deliberate overrun
  shows that the guards catch one."""
import os
import subprocess
import sys

import pytest

from conftest import ROOT

LIBDIR = os.path.join(ROOT, "revrand_amd", "lib")
ASAN_LIB = os.path.join(LIBDIR, "librevrand_hip_asan.so")
DEBUG_LIB = os.path.join(LIBDIR, "librevrand_hip_debug.so")
RAGGED = ["tests/test_gpu_rff.py::test_tiny_and_ragged_shapes_end_to_end", "tests/test_gpu_rff.py::test_transform_shapes_vs_oracle",
          "tests/test_gpu_rff.py::test_gram_vs_oracle", "tests/test_gpu_rff.py::test_gram_f64_vs_oracle",
          "tests/test_gpu_fastfood.py", "tests/test_gpu_slm.py::test_concat_second_pass_and_predict_vs_oracle",
          "tests/test_gpu_slm.py::test_second_pass_and_predict_vs_oracle", "tests/test_gpu_large_xdim.py",
          "tests/test_gpu_parity_r2.py::test_gram_with_a_ragged_last_column_block",
          "tests/test_gpu_parity_r2.py::test_predictive_variance_is_a_sum_of_squares_for_badly_scaled_covariances",
          # round 3: the products fused with their consumers (partial row tiles, Xdim below / above 32)
          "tests/test_gpu_slm.py::test_second_pass_product_fused_with_its_contraction_equals_the_two_pass_route",
          "tests/test_gpu_glm.py::test_edphi_product_fused_with_its_contraction_equals_the_two_pass_route",
          "tests/test_gpu_glm.py::test_first_product_with_the_likelihood_terms_as_its_epilogue_equals_the_three_pass_route",
          # round 4: the posterior's panel pipeline at config 3's width (65 panels, ragged last one) and its failure path
          "tests/test_gpu_posterior.py::test_posterior_vs_oracle_solve_posdef[8257-default]",
          "tests/test_gpu_posterior.py::test_not_positive_definite_in_a_late_panel_is_reported_and_leaves_nothing_in_flight[8257-8256-default]",
          # round 4: `predict` from the feature kernel alone (no feature-major output), ragged row counts; the paired
          # triangular product with the diagonal blocks' zero quarters skipped runs under the two predict tests above
          "tests/test_gpu_slm.py::test_predict_of_a_random_kernel_basis_comes_from_the_feature_kernel_alone",
          # round 5: the resident SVI loop (per-child tables, two feature matrices, the second stream), ragged minibatches
          "tests/test_gpu_resident_sgd.py::test_concatenation_of_fourier_and_linear_children",
          "tests/test_gpu_resident_sgd.py::test_resident_loop_equals_host_loop",
          # round 6: the in-process device group (every launch checked for "current device == the stream's device"), on
          # distinct GPUs where the box has them; the reference-pinned GLM fits through both loops
          "tests/test_gpu_multigpu.py::test_sharded_elbo_equals_the_one_context_elbo",
          "tests/test_gpu_multigpu_devices.py::test_one_member_group_under_rccl_runs_the_grouped_calls",
          "tests/test_gpu_multigpu_devices.py::test_elbo_with_devices_for_every_fit_state",
          "tests/test_gpu_glm_fit.py::test_fit_equals_the_references_fit[gaussian_cat_bs10_ns5-fused loop]",
          "tests/test_gpu_glm_fit.py::test_fit_equals_the_references_fit[binomial_cat_bs10_ns3-fused loop]",
          "tests/test_gpu_glm_fit.py::test_fit_equals_the_references_fit[poisson_ard_bs64f_ns5-resident loop]",
          "tests/test_gpu_fused_svi.py::test_shapes_across_the_tiles_of_the_matrix_core_products",
          "tests/test_gpu_resident_group.py::test_a_member_without_rows_of_a_minibatch_follows_the_others[two streams]",
          "tests/test_gpu_resident_group.py::test_group_resident_fit_equals_the_one_context_fit[two streams-gaussian-cat-devices2-host]",
          "tests/test_gpu_resident_group.py::test_group_resident_fit_equals_the_one_context_fit[one stream-binomial-iso-devices1-device]",
          "tests/test_gpu_resident_group.py::test_group_resident_fit_equals_the_one_context_fit[two streams-poisson-gm-devices4-host]",
          "tests/test_gpu_resident_sgd.py::test_spectral_mixture_children_run_resident[two streams-12-gaussian]",
          # every route of the GLM step's products and of `project`, bit for bit on integer data (ragged rows, F and S)
          "tests/test_gpu_glm_routes.py::test_project_is_exact_on_every_route",
          "tests/test_gpu_glm_routes.py::test_step_is_exact_on_every_route",
          "tests/test_gpu_glm_routes.py::test_step_sequence_is_exact",
          # every instance of the FastFood chain kernels on integer data and at exactly known phases: scalar and vector
          # accesses, part waves, one to nine rows, offset pointers and leading dimensions into sentinel-filled buffers
          "tests/test_gpu_fastfood_exact.py",
          # every route of the Gram launchers (f32, f64, split 16-bit) bit for bit on exact data: ragged rows and widths, the
          # rider column, prefilled accumulators, one feature matrix through shrinking and growing row counts
          "tests/test_gpu_gram_exact.py::test_small_widths_are_exact",
          "tests/test_gpu_gram_exact.py::test_main_kernel_routes_are_exact",
          "tests/test_gpu_gram_exact.py::test_ragged_last_block_is_exact",
          "tests/test_gpu_gram_exact.py::test_tile_map_routes_are_exact",
          "tests/test_gpu_gram_exact.py::test_k_split_geometries_are_exact",
          "tests/test_gpu_gram_exact.py::test_gram_adds_to_the_upper_triangle_only",
          "tests/test_gpu_gram_exact.py::test_deterministic_mode_is_exact_and_repeats",
          "tests/test_gpu_gram_exact.py::test_one_feature_matrix_through_changing_row_counts",
          "tests/test_gpu_gram_exact.py::test_dense_gram_f32_is_exact",
          "tests/test_gpu_gram_exact.py::test_dense_gram_f64_is_exact",
          "tests/test_gpu_gram_exact.py::test_feature_matrix64_is_exact",
          "tests/test_gpu_gram_exact.py::test_split_engine_three_products_are_exact",
          "tests/test_gpu_gram_exact.py::test_split_engine_four_products_are_exact",
          # every route of the device posterior bit for bit on exact dyadic data: one to ten panels and 35, ragged last panels,
          # the cooperative kernel, refusals in every panel, the work space re-sized, the prediction factor
          "tests/test_gpu_posterior_exact.py::test_pipeline_is_exact",
          "tests/test_gpu_posterior_exact.py::test_scratch_follows_the_size",
          "tests/test_gpu_posterior_exact.py::test_cooperative_kernel_is_exact",
          "tests/test_gpu_posterior_exact.py::test_threshold_is_exact_and_a_refusal_leaves_nothing_behind",
          "tests/test_gpu_posterior_exact.py::test_variance_factor_is_exact",
          "tests/test_gpu_posterior_exact.py::test_variance_factor_falls_back_to_the_quadratic_form",
          # every route of the second pass and of predict_moments bit for bit on integer and quarter-turn data: one row to
          # partial last row tiles, children off the tile grid, Xdim 5 .. 130, shrinking row counts, row chunks, float64
          "tests/test_gpu_pass2_exact.py::test_quarter_turn_features_are_exact",
          "tests/test_gpu_pass2_exact.py::test_gradient_pass_is_exact",
          "tests/test_gpu_pass2_exact.py::test_gradient_pass_with_more_row_tiles_than_workgroups_is_exact",
          "tests/test_gpu_pass2_exact.py::test_gradient_pass_over_the_input_dimensions_is_exact",
          "tests/test_gpu_pass2_exact.py::test_gradient_pass_with_float64_inputs_is_exact",
          "tests/test_gpu_pass2_exact.py::test_gradient_pass_in_deterministic_mode_is_exact_and_repeats",
          "tests/test_gpu_pass2_exact.py::test_one_feature_matrix_through_shrinking_row_counts",
          "tests/test_gpu_pass2_exact.py::test_gradient_pass_with_a_child_that_wrote_its_transpose",
          "tests/test_gpu_pass2_exact.py::test_prediction_is_exact",
          "tests/test_gpu_pass2_exact.py::test_one_feature_matrix_predicts_shrinking_row_counts",
          "tests/test_gpu_pass2_exact.py::test_split_engines_are_exact",
          "tests/test_gpu_pass2_exact.py::test_feature_matrix64_is_exact",
          "tests/test_gpu_pass2_exact.py::test_basis_gradient_pass_is_exact",
          "tests/test_gpu_pass2_exact.py::test_basis_stored_routes_are_exact",
          "tests/test_gpu_pass2_exact.py::test_basis_prediction_is_exact"]


def _asan_runtime():
    for cc in ("/opt/rocm/bin/hipcc", "/opt/rocm/lib/llvm/bin/clang"):
        if os.path.exists(cc):
            p = subprocess.run([cc, "-print-file-name=libclang_rt.asan-x86_64.so"], capture_output=True, text=True).stdout.strip()
            if os.path.isabs(p) and os.path.exists(p):
                return p
    return None


def _pytest_with(lib, args, preload=None, timeout=1500):
    env = dict(os.environ, REVRAND_HIP_LIB=lib)
    if preload:
        env.update(LD_PRELOAD=preload, ASAN_OPTIONS="detect_leaks=0:protect_shadow_gap=0:abort_on_error=1")
        # The (uninstrumented) HIP runtime must tolerate a preloaded ASan runtime: the copy bundled with the torch wheel
        # does; /opt/rocm's aborts inside its own initialisation under the preload (ROCm ships separate ASan builds of its
        # libraries for that).  What is under test is the host side of librevrand_hip_asan.so, not the runtime.
        try:
            import importlib.util
            if importlib.util.find_spec("torch") is not None:
                env["RR_HIP_RUNTIME"] = "torch"
        except (ImportError, ValueError):
            pass
    return subprocess.run([sys.executable, "-m", "pytest", "-q", "-x", "-p", "no:cacheprovider"] + args, cwd=ROOT, env=env,
                          capture_output=True, text=True, timeout=timeout)


def test_asan_build_passes_the_abi_checks():
    rt = _asan_runtime()
    if not os.path.exists(ASAN_LIB) or rt is None:
        pytest.skip("make -C revrand_amd/csrc asan has not been run")
    # the ABI checks, and the one host-only entry point with real work in it (rr_legacy_randn: worker threads, scratch)
    r = _pytest_with(ASAN_LIB, ["tests/test_abi.py", "tests/test_host_logic.py::test_library_generator_reproduces_numpy_legacy_randn",
                                "tests/test_host_logic.py::test_library_generator_reproduces_numpy_legacy_permutation",
                                "-m", "not gpu"], preload=rt, timeout=900)
    assert r.returncode == 0 and "AddressSanitizer" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_asan_build_runs_the_ragged_shape_tests():
    rt = _asan_runtime()
    if not os.path.exists(ASAN_LIB) or rt is None:
        pytest.skip("make -C revrand_amd/csrc asan has not been run")
    r = _pytest_with(ASAN_LIB, RAGGED[:3] + RAGGED[4:5] + ["-m", "gpu"], preload=rt)
    # every test passed, and no ASan report has a frame of this library in it.  (The HSA runtime bundled with torch
    # occasionally trips ASan inside libhsa-runtime64.so while the process exits, after the summary line: not ours.)
    import re
    assert re.search(r"\b\d+ passed\b", r.stdout) and not re.search(r"\b(failed|error)\b", r.stdout), \
        (r.stdout[-2500:], r.stderr[:3000], r.stderr[-1500:])
    reports = (r.stdout + r.stderr).split("ERROR: AddressSanitizer")[1:]
    assert not any("librevrand_hip" in rep for rep in reports), (r.stdout + r.stderr)[-4000:]


@pytest.mark.gpu
@pytest.mark.timeout(1800)
def test_bounds_build_runs_the_ragged_shape_tests():
    if not os.path.exists(DEBUG_LIB):
        pytest.skip("make -C revrand_amd/csrc debug has not been run")
    r = _pytest_with(DEBUG_LIB, RAGGED + ["-m", "gpu"])
    assert r.returncode == 0 and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-2500:], r.stderr[-3000:])


@pytest.mark.gpu
def test_bounds_build_catches_an_overrun():
    if not os.path.exists(DEBUG_LIB):
        pytest.skip("make -C revrand_amd/csrc debug has not been run")
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "from revrand_amd import _hip\n"
        "dev = _hip.get_device()\n"
        "assert dev.lib.rr_build_flags() & 1\n"
        "buf = dev.malloc(1000)\n"
        "dev.memset(buf, 1000); dev.sync()            # in bounds: fine\n"
        "_hip._check(dev.lib, dev.lib.rr_memset(dev.ctx, buf.ptr, 0, 1016))   # 16 bytes past the end\n"
        "try:\n"
        "    dev.sync()\n"
        "except _hip.HipError as e:\n"
        "    assert 'RR_BOUNDS' in str(e) and 'offset 1000' in str(e), str(e)\n"
        "    print('caught')\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB), capture_output=True,
                       text=True, timeout=600)
    assert "caught" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])


@pytest.mark.gpu
def test_bounds_build_checks_the_device_of_every_launch():
    """-DRR_BOUNDS wraps every kernel launch of the library in a check that the calling thread's current HIP device is the
    device of the stream launched on (rr_internal.h) -- what the in-process device group relies on and a one-GPU box cannot
    show broken.  A sharded `_elbo` (members on distinct GPUs when the box has two) makes thousands of such launches from
    several host threads: all checked, none in violation (a violation fails the next synchronisation)."""
    if not os.path.exists(DEBUG_LIB):
        pytest.skip("make -C revrand_amd/csrc debug has not been run")
    code = (
        "import sys; sys.path.insert(0, %r)\n"
        "import numpy as np\n"
        "from revrand_amd import _hip, multigpu\n"
        "import revrand_amd.basis_functions as bs\n"
        "from revrand_amd.slm import StandardLinearModel\n"
        "lib = _hip.load_library()\n"
        "assert lib.rr_build_flags() & 1 and lib.rr_debug_launch_checks() == 0\n"
        "v = multigpu.visible_devices()\n"
        "devices = list(range(min(v, 4))) if v >= 2 else [0, 0, 0]\n"
        "rs = np.random.RandomState(0)\n"
        "X = rs.randn(20000, 5).astype(np.float32); y = np.sin(X[:, 0]).astype(np.float32)\n"
        "slm = StandardLinearModel(bs.RandomRBF(nbases=64, Xdim=5, random_state=1) + bs.LinearBasis(), nstarts=0, maxiter=3,\n"
        "                          devices=devices).fit(X, y)\n"
        "slm.predict_moments(X[:3000])\n"
        "multigpu.get_group(devices).sync()\n"
        "n = lib.rr_debug_launch_checks()\n"
        "assert n > 100, n\n"
        "print('checked', n, 'launches on', devices)\n" % ROOT)
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB), capture_output=True,
                       text=True, timeout=900)
    assert "checked" in r.stdout and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-1500:], r.stderr[-3000:])


@pytest.mark.gpu
def test_bounds_build_counts_the_kernel_each_route_takes():
    """One GLM step (or projection) per case of tests/test_gpu_glm_routes.py under the bounds-checking build, which counts
    launches per kernel (rr_debug_kernel_launches): each product ran on the kernel the module's route table names for this
    device's CU count, and no other GEMM kernel ran -- the table stays honest if a rule of fm_gemm or glm_pipeline changes."""
    if not os.path.exists(DEBUG_LIB):
        pytest.skip("make -C revrand_amd/csrc debug has not been run")
    code = (
        "import json, sys; sys.path[:0] = [%r, %r, %r]\n"
        "import test_gpu_glm_routes as R\n"
        "print('CENSUS', json.dumps(R.census()))\n" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB),
                       capture_output=True, text=True, timeout=900)
    lines = [l for l in r.stdout.splitlines() if l.startswith("CENSUS ")]
    assert r.returncode == 0 and lines and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-1500:], r.stderr[-3000:])
    import json
    rows = json.loads(lines[-1][len("CENSUS "):])
    bad = []
    for label, cu, got, want in rows:
        print("%-36s cu=%d %s" % (label, cu, " ".join("%s=%d" % (k.replace("_f32_kernel", "").replace("_kernel", ""), v)
                                                      for k, v in sorted(got.items()) if v)))
        if got != want:
            bad.append((label, got, want))
    assert len(rows) >= 30 and not bad, bad


@pytest.mark.gpu
def test_bounds_build_counts_the_second_pass_kernel_each_route_takes():
    """One second pass or prediction per case of tests/test_gpu_pass2_exact.py's census under the bounds-checking build,
    which counts launches per kernel: the fused and the stored products, the pair kernel, the contraction, row and
    feature-major kernels, the split engines' and the float32 transposes ran as often as `pass2_route`, `predict_route`
    and `basis_route` predict for this device's CU count and no other of them ran; every counted call was exact as well.
    The counter drops template arguments: NXB = 1 | 2 | 4 of rr_gemm_gradt_f32_kernel and DM of rr_grad_t_kernel are
    not told apart here (that module's coverage test and exact results hold them).  The child shares the Gram module's
    guard: it is not started after a child that failed, reported a bounds violation or hung."""
    if not os.path.exists(DEBUG_LIB):
        pytest.skip("make -C revrand_amd/csrc debug has not been run")
    import test_gpu_gram_exact as E
    import test_gpu_pass2_exact as S
    rows = E.guarded_child("the second-pass census", S.CHILD_CODE + "print('CENSUS', json.dumps(S.census()))\n",
                           {"REVRAND_HIP_LIB": DEBUG_LIB}, "CENSUS", timeout=900, forbidden=("RR_BOUNDS",))
    bad, ran = [], set()
    for label, cu, got, want, wrong in rows:
        print("%-56s cu=%d %s" % (label, cu, " ".join("%s=%d" % (k.replace("rr_", "").replace("_kernel", ""), v)
                                                      for k, v in sorted(got.items()) if v)))
        ran |= {k for k, v in got.items() if v}
        if got != want or wrong:
            bad.append((label, {k: (got[k], want[k]) for k in got if got[k] != want[k]}, wrong))
    assert len(rows) >= 150 and not bad, bad[:10]
    assert {"rr_gemm_gradt_f32_kernel", "rr_gemm_tn_f32_kernel", "rr_gemm_pair_f32_kernel", "rr_grad_t_kernel", "rr_err_kernel",
            "rr_rowdot_kernel", "rr_rowvec_kernel", "rr_transpose_f32_kernel", "rr_rff_features_t4_kernel", "rr_c64_to_c32_kernel",
            "rr_split_bf16_kernel", "rr_syrk_b16w4_kernel", "rr_transpose_f64_kernel", "rr_rows64_kernel", "rr_err64_kernel",
            "rr_grad_t64_kernel"} <= ran, sorted(ran)


def _gram_variants():
    import test_gpu_gram_exact as E
    return [{}] + E.AB_VARIANTS


@pytest.mark.gpu
@pytest.mark.parametrize("variant", _gram_variants(), ids=lambda v: ",".join("%s=%s" % kv for kv in v.items()) or "default")
def test_bounds_build_counts_the_gram_kernel_each_route_takes(variant):
    """One Gram per case of tests/test_gpu_gram_exact.py's census under the bounds-checking build, which counts launches per
    kernel: every SYRK, conversion, rider and gemv kernel ran as often as the module's route tables predict for this
    device's CU count and no other one ran -- by default (the two cases of hundreds of megabytes included), and once per A/B
    variable the launcher reads at process start.  The census shows the switch where it changes a kernel's name:
    RR_SYRK_NO_DIAG16 (rr_syrk_f32_diag_kernel), RR_SYRK_MERGE_DIAG (rr_syrk_f32_merged_kernel), RR_SYRK_STAGGER (the flat,
    flatstag and buf kernels) and RR_SYRK_SMALL=0 (no small kernel).  It cannot show it for RR_SYRK_DIAG_KB=64, which picks
    rr_syrk_f32_diag16_kernel<64> -- the launch counter drops template arguments --, nor for RR_SYRK_SPLIT_SEARCH=0, which
    changes split counts and no kernel: for those two the run holds only that the same kernels ran, and their results are
    held by test_gpu_gram_exact.py::test_ab_variants_are_exact.  The children run one after another and share that
    module's guard: none is started after a child, here or there, that failed, reported a bounds violation or hung."""
    if not os.path.exists(DEBUG_LIB):
        pytest.skip("make -C revrand_amd/csrc debug has not been run")
    import test_gpu_gram_exact as E
    rows = E.guarded_child("the census under %s" % (variant or "the default switches",), "print('CENSUS', json.dumps(E.census(big=%r)))\n"
                           % (not variant), dict(variant, REVRAND_HIP_LIB=DEBUG_LIB), "CENSUS", timeout=900, forbidden=("RR_BOUNDS",))
    bad, ran = [], set()
    for label, cu, got, want in rows:
        print("%-40s cu=%d %s" % (label, cu, " ".join("%s=%d" % (k.replace("rr_", "").replace("_kernel", ""), v)
                                                      for k, v in sorted(got.items()) if v)))
        ran |= {k for k, v in got.items() if v}
        if got != want:
            bad.append((label, got, want))
    assert len(rows) >= 55 and not bad, bad
    switched = {"RR_SYRK_NO_DIAG16": "rr_syrk_f32_diag_kernel", "RR_SYRK_MERGE_DIAG": "rr_syrk_f32_merged_kernel"}
    switched.update({"RR_SYRK_STAGGER": ["rr_syrk_f32_flat_kernel", "rr_syrk_f32_flatstag_kernel", "rr_syrk_f32_buf_kernel"][int(v)]
                     for k, v in variant.items() if k == "RR_SYRK_STAGGER"})
    for k in variant:
        assert k not in switched or switched[k] in ran, (variant, sorted(ran))
    if variant.get("RR_SYRK_SMALL") == "0":
        assert "rr_syrk_f32_small_kernel" not in ran


def _posterior_variants():
    import test_gpu_posterior_exact as P
    return [{}] + P.VARIANTS


@pytest.mark.gpu
@pytest.mark.parametrize("variant", _posterior_variants(), ids=lambda v: ",".join("%s=%s" % kv for kv in sorted(v.items())) or "default")
def test_bounds_build_counts_the_posterior_kernel_each_route_takes(variant):
    """One rr_posterior_dev per size and mode of tests/test_gpu_posterior_exact.py's census (one to ten panels, the cooperative
    kernel, the prediction factor in both forms) under the bounds-checking build, which counts launches per kernel: every
    diagonal-block, product, SYRK, row and factor kernel ran as often as the module's restated rules predict and no other
    one -- by default, and once per switch that rr_posterior_dev, launch_chol_diag and rr_launch_gemm_tn_f64 read at process
    start.  Where a switch changes a kernel's name the census shows it: the two RR_CHOL_DIAG kernels ran and the default one
    did not; with RR_GEMM64_K128=0 no K = 128 launch appears.  Where it changes only counts (pairing, look-ahead, one stream)
    test_cases_cover_every_route asserts that the prediction differs from the default's, so `got == want` is not vacuous;
    RR_POSDEF_EARLY_CHECK changes no launch at all and is held by its exact results alone.  Every call of the census is
    also exact.  The children share the Gram module's guard: none is started after one that failed, reported a bounds
    violation or hung."""
    if not os.path.exists(DEBUG_LIB):
        pytest.skip("make -C revrand_amd/csrc debug has not been run")
    import test_gpu_gram_exact as E
    import test_gpu_posterior_exact as P
    code = P.CHILD_CODE % (sorted(variant),) + "print('CENSUS', json.dumps(P.census()))\n"
    rows = E.guarded_child("the posterior census under %s" % P.variant_id(variant), code, dict(variant, REVRAND_HIP_LIB=DEBUG_LIB),
                           "CENSUS", timeout=2 * P.CHILD_TIMEOUT, forbidden=("RR_BOUNDS",))
    bad, ran = [], set()
    for label, got, want, wrong in rows:
        print("%-24s %s" % (label, " ".join("%s=%d" % (k.replace("rr_", "").replace("_kernel", ""), v) for k, v in sorted(got.items()) if v)))
        ran |= {k for k, v in got.items() if v}
        if got != want or wrong:
            bad.append((label, got, want, wrong))
    assert [row[0] for row in rows] == P.census_labels() and len(rows) == 25 and not bad, bad
    chol = P.chol_kernel(variant)
    assert chol in ran and not (set(P.CHOL_KERNELS) - {chol}) & ran, sorted(ran)
    assert ("rr_gemm_tn_f64_k128_kernel" in ran) == (variant.get("RR_GEMM64_K128") != "0") and "rr_gemm_tn_f64_kernel" in ran
    assert {"rr_posterior_coop_kernel", "rr_reverse_pad_kernel", "rr_ul_factor_f32_kernel", "rr_c64_to_c32_kernel",
            "rr_syrk_f64_kernel", "rr_syrk_f64_diag_kernel", "rr_posterior_rows_kernel"} <= ran


@pytest.mark.gpu
def test_bounds_build_counts_the_fastfood_instance_each_case_runs():
    """Every chain-kernel call of tests/test_gpu_fastfood_exact.py (census_runs: the case lists and the rows-per-block, grid
    clamp, chunk seam and feature-matrix cases) under the bounds-checking build, which counts each FastFood launch under
    an identifier naming its instance (family / registers / mode / vec or scalar / full or partial): the case ran the instance
    the module's table names and no other FastFood instance -- by default, and under RR_FASTFOOD_OLD=1 (the lane-minor kernel
    at 16 <= d2 <= 256).  Together the cases run every reachable instance."""
    if not os.path.exists(DEBUG_LIB):
        pytest.skip("make -C revrand_amd/csrc debug has not been run")
    import json
    code = (
        "import json, sys; sys.path[:0] = [%r, %r, %r]\n"
        "import test_gpu_fastfood_exact as E\n"
        "print('CENSUS', json.dumps(E.census()))\n" % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")))
    ran, bad = {}, []
    for extra in ({}, {"RR_FASTFOOD_OLD": "1"}):
        env = dict(os.environ, REVRAND_HIP_LIB=DEBUG_LIB, **extra)
        if not extra:
            env.pop("RR_FASTFOOD_OLD", None)
        r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
        lines = [l for l in r.stdout.splitlines() if l.startswith("CENSUS ")]
        assert r.returncode == 0 and lines and "RR_BOUNDS" not in (r.stdout + r.stderr), (r.stdout[-1500:], r.stderr[-3000:])
        for label, got, want in json.loads(lines[-1][len("CENSUS "):]):
            if set(got) != {want}:
                bad.append((label, got, want))
            ran.setdefault(want, label)
    for name in sorted(ran):
        print("%-52s %s" % (name, ran[name]))
    import test_gpu_fastfood_exact as E
    reachable = E.reachable_idents()
    assert not bad, bad
    assert set(ran) == reachable, (sorted(reachable - set(ran)), sorted(set(ran) - reachable))


def _rff_variants():
    import rff_cases as R
    return [None] + list(R.SWITCHES)


@pytest.mark.gpu
@pytest.mark.parametrize("switch", _rff_variants(), ids=lambda s: s or "default")
def test_bounds_build_counts_the_feature_kernel_each_route_takes(switch):
    """One call per census case of tests/test_gpu_rff_exact.py under the bounds-checking build, which counts launches per
    kernel: the matrix-core, VALU, large-Xdim (transpose, GEMM with and without the cos / sin epilogue, float64 phase, trig),
    gradient, spectral-mixture and rescaling kernels ran as often as `feature_route` of tests/rff_cases.py predicts for this
    device's CU count and no other of them ran -- by default, and once per switch read at process start (RR_FEATURES_NO_MFMA,
    RR_FEATURES_NO_MFMA64: no launch of the kernel switched off; RR_PREPARE_ON_HOST: no rescaling kernel).  Every counted call
    also met its per-element bound and left the sentinel around its block.  The counter drops template arguments: DMAX, the
    (x, out) type pairs and HAS_Y / WT are not told apart here -- tests/test_rff_cases_host.py's coverage test and the results
    hold them.  The children share the Gram module's guard: none is started after one that failed, reported a bounds
    violation or hung."""
    if not os.path.exists(DEBUG_LIB):
        pytest.skip("make -C revrand_amd/csrc debug has not been run")
    import test_gpu_gram_exact as E
    import test_gpu_rff_exact as X
    env = {"REVRAND_HIP_LIB": DEBUG_LIB}
    if switch:
        env[switch] = "1"
    rows = E.guarded_child("the feature-kernel census under %s" % (switch or "the default switches"),
                           X.CHILD_CODE + "print('CENSUS', json.dumps(X.census(%r)))\n" % (switch,), env, "CENSUS", timeout=900,
                           forbidden=("RR_BOUNDS",))
    bad, ran = [], set()
    for label, cu, got, want, wrong in rows:
        print("%-44s cu=%d %s" % (label, cu, " ".join("%s=%d" % (k.replace("rr_", "").replace("_kernel", ""), v)
                                                      for k, v in sorted((got or {}).items()) if v)))
        ran |= {k for k, v in (got or {}).items() if v}
        if got != want or wrong:
            bad.append((label, {k: (got[k], want[k]) for k in want if got is None or got[k] != want[k]} if got else None, wrong))
    assert len(rows) >= (300 if switch is None else 4) and not bad, bad[:10]
    if switch is None:
        assert {"rr_rff_features_mfma_kernel", "rr_rff_features_mfma64_kernel", "rr_rff_transform_kernel", "rr_rff_grad_kernel",
                "rr_rff_features_kernel", "rr_rff_grad_p_kernel", "rr_xt_kernel", "rr_gemm_trig_f32_kernel", "rr_gemm_tn_small_f32_kernel",
                "rr_phase_f64_kernel", "rr_trig_kernel", "rr_scale_w_kernel", "rr_scale_w_dev_kernel", "rr_gm_transform_kernel",
                "rr_gm_grad_kernel"} <= ran, sorted(ran)
    elif switch == "RR_FEATURES_NO_MFMA":
        assert "rr_rff_features_mfma_kernel" not in ran and "rr_rff_features_kernel" in ran
    elif switch == "RR_FEATURES_NO_MFMA64":
        assert "rr_rff_features_mfma64_kernel" not in ran and "rr_rff_features_kernel" in ran
    else:
        assert "rr_scale_w_kernel" not in ran
