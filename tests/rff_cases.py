"""Cases, references and per-element bounds for every route of the random Fourier feature kernels (rr_rff.hip); host only,
imported by tests/test_rff_cases_host.py (CPU) and tests/test_gpu_rff_exact.py (GPU).

Three things live here.

* The route table.  `feature_route` restates which kernels a call launches and how often: rr_features_mfma_ok /
  rr_features_mfma_launch (alignment, the `Pt` conditions, the tiles-per-workgroup halving against the CU count, RR_FEAT_TPB,
  the 65535 grid clamp), rr_features_mfma64_launch, launch_transform (whole 32- or 16-row tiles on the matrix cores, the
  remaining rows on rr_rff_transform_kernel, which stages x through LDS in float64), launch_grad, large_features (Xdim > 128:
  GEMM with the cos / sin epilogue for float32 features, GEMM + rr_trig_kernel for float64 output, rr_phase_f64_kernel +
  rr_trig_kernel in float64 arithmetic, sub-chunks of RR_LG_ROWS rows), the feature pass of launch_gram,
  rr_features_rowmajor_f32 / _f64 (FeatureMatrix(64).put_rff) and the three rescaling routes of the length scales
  (rr_scale_w_kernel, host scaling under RR_PREPARE_ON_HOST or Xdim > 128, rr_basis_prepare_dev's rr_scale_w_dev_kernel).

* Family A, dyadic phases: W = 2 pi Q l_i / 2^k with integer Q, l_i a power of two, x integer in [-8, 8].  The library's
  Ws = W (inv2pi / l) rounds to Q / 2^k exactly in float32 (asserted per data set), every partial sum of the float32
  projection is an integer multiple of 2^-k below 2^24 of them and therefore exact in any order, on the matrix cores or the
  VALU; the reference reduces sum_i x_i Q_if mod 2^k in integers.  What is left is the error of the sine / cosine and of the
  scale multiply: nothing is granted for the phase in float32 arithmetic.

* Family B, real-valued data: x, W continuous, length scales not dyadic, scaled to at most two revolutions of sum_i |x_i Ws_if|
  so that the forward bound of the projection stays well below the old normwise tolerance even at d = 128.  The reference
  accumulates the phase in long double from W / (2 pi l), not from the library's rounded table.

Every term of `phi_bound` / `grad_bound` / `bty_bound` is derived next to the code line it accounts for; the one measured
figure is SINCOS_F32_MAX_ERR of tests/test_gpu_fastfood_exact.py (tools/probes/sincos_probe.hip, docs/KERNELS.md 3.7), used
with that module's factor of two.

Out of scope: the split 16-bit feature output of the Gram engines (`fused_pb`: held by test_gpu_gram_engines.py and the
split-engine cases of test_gpu_gram_exact.py), rr_rff_grad_contract, and the feature-major kernels of rr_elbo.hip, which
tests/test_gpu_pass2_exact.py holds at quarter turns."""
from collections import Counter, namedtuple
from types import SimpleNamespace

import numpy as np

from test_gpu_fastfood_exact import PHI_F32_BOUND, PHI_F64_BOUND, SINCOS_F32_MAX_ERR

INV2PI = 0.15915494309189533576888  # the library's literal (rr_basis_prepare, rr_scale_w_kernel)
TWO_PI = 6.283185307179586476925
TWO_PI_L = 2 * np.arccos(np.longdouble(-1))
U32, U64 = 2.0 ** -24, 2.0 ** -53
NP = {"f32": np.float32, "f64": np.float64}
RR_LG_ROWS = 131072   # rr_rff.hip
CB = {8: 4, 16: 4, 32: 4, 64: 2, 128: 1}   # column blocks per wave of the two matrix-core kernels (RR_FM / RR_FM64)
DMAXES = (8, 16, 32, 64, 128)
SENTINEL = {4: np.uint32(0xC2F7A5A5), 8: np.uint64(0xC2F7A5A5C2F7A5A5)}

FEATURE_KERNELS = ("rr_rff_features_mfma_kernel", "rr_rff_features_mfma64_kernel", "rr_rff_transform_kernel", "rr_rff_grad_kernel",
                   "rr_rff_features_kernel", "rr_rff_grad_p_kernel", "rr_xt_kernel", "rr_gemm_trig_f32_kernel",
                   "rr_gemm_tn_small_f32_kernel", "rr_gemm_tn_f32_kernel", "rr_gemm_tn_mid_f32_kernel", "rr_phase_f64_kernel",
                   "rr_trig_kernel", "rr_scale_w_kernel", "rr_scale_w_dev_kernel", "rr_gm_transform_kernel", "rr_gm_grad_kernel")


# ---- the route table ----------------------------------------------------------------------------------------------------------
def pick_dmax(d):
    """rr_pick_dmax."""
    for m in DMAXES:
        if d <= m:
            return m
    return 0


def basis_dims(d, n):
    """(large, dpad, npad) as rr_rff_create lays the basis out."""
    dpad = pick_dmax(d)
    if dpad:
        return False, dpad, (n + 127) // 128 * 128
    return True, (d + 127) // 128 * 128, (n + 255) // 256 * 256


def _cdiv(a, b):
    return (a + b - 1) // b


def mfma_grid(mpad, n, dpad, cu, env):
    """(column groups, grid.y, tiles per workgroup) of rr_features_mfma_launch (RR_FM)."""
    ntiles, cg, tpb = _cdiv(mpad, 32), _cdiv(n, 32 * CB[dpad]), 64
    while tpb > 16 and cg * _cdiv(ntiles, tpb) < 4 * cu:
        tpb >>= 1
    while tpb > 4 and cg * _cdiv(ntiles, tpb) < cu:
        tpb >>= 1
    if "RR_FEAT_TPB" in env:
        tpb = int(env["RR_FEAT_TPB"])
    if _cdiv(ntiles, tpb) > 65535:
        tpb = (ntiles + 65534) // 65535
    return cg, _cdiv(ntiles, tpb), tpb


def mfma64_grid(mpad, n, dpad, cu):
    """The same of rr_features_mfma64_launch (RR_FM64)."""
    ntiles, cg, tpb = _cdiv(mpad, 16), _cdiv(n, 16 * CB[dpad]), 128
    while tpb > 4 and cg * _cdiv(ntiles, tpb) < 8 * cu:
        tpb >>= 1
    if _cdiv(ntiles, tpb) > 65535:
        tpb = (ntiles + 65534) // 65535
    return cg, _cdiv(ntiles, tpb), tpb


def valu_transform_grid(N, n, cu):
    """(frequency blocks, grid.y, rows per block) of launch_transform's rr_rff_transform_kernel."""
    fb = _cdiv(n, 256)
    rpb = min(max(_cdiv(N * fb, cu * 16), 16), 1024)
    if _cdiv(N, rpb) > 65535:
        rpb = (N + 65534) // 65535
    return fb, _cdiv(N, rpb), rpb


def valu_rows_grid(N, n, rpb):
    """launch_grad (rpb = 16) and the rr_rff_features_kernel launches (rpb = 256): fixed rows per block, clamped to 65535."""
    if _cdiv(N, rpb) > 65535:
        rpb = (N + 65534) // 65535
    return _cdiv(n, 256), _cdiv(N, rpb), rpb


def gemm_tn_kernel(K, M, N, cu):
    """fm_gemm with allow_mid = false (rr_launch_gemm_tn_f32): the 32 x 32 kernel for small products, else the tile kernel."""
    return "rr_gemm_tn_small_f32_kernel" if K * M * N <= 1 << 27 and M // 32 < 65536 else "rr_gemm_tn_f32_kernel"


def det_reduce(nslots, count):
    """rr_det_reduce: one kernel, or 64 groups first."""
    if nslots >= 512 and count >= 256:
        return Counter(rr_det_group_kernel=1, rr_det_reduce_kernel=1)
    return Counter(rr_det_reduce_kernel=1)


class Route(object):
    def __init__(self):
        self.kernels, self.rows, self.grids, self.error = Counter(), [], [], None

    def add(self, kernel, row, grid=None, count=1):
        self.kernels[kernel] += count
        self.rows.append(row)
        if grid is not None:
            self.grids.append((kernel,) + tuple(grid))

    def counts(self, names=FEATURE_KERNELS):
        return {k: int(self.kernels.get(k, 0)) for k in names}


def _pair(x, o):
    return "%s->%s" % (x, o)


def _large(R, arith, x_dtype, out_dtype, m, mpad, dpad, npad, n, with_y, cu):
    """large_features<TX, TC, TO>: per sub-chunk of RR_LG_ROWS rows."""
    sub = min(_cdiv(mpad, 256) * 256, RR_LG_ROWS)
    for s0 in range(0, mpad, sub):
        rows_out = min(mpad - s0, sub)
        rows_in = max(0, min(m - s0, sub))
        if rows_in > 0:
            r256 = _cdiv(rows_in, 256) * 256
            if arith == "f32":
                R.add("rr_xt_kernel", "large/xt/%s" % x_dtype)
                if out_dtype == "f32":
                    R.add("rr_gemm_trig_f32_kernel", "large/gemm_trig/%s%s" % (_pair(x_dtype, out_dtype), "/has_y" if with_y else ""))
                    continue
                R.add(gemm_tn_kernel(dpad, r256, npad, cu), "large/gemm+trig/%s" % _pair(x_dtype, out_dtype))
            else:
                R.add("rr_phase_f64_kernel", "large/phase64+trig/%s%s" % (_pair(x_dtype, out_dtype), "/has_y" if with_y else ""))
        fb = _cdiv(n, 256)
        rpb = min(max(_cdiv(rows_out * fb, cu * 16), 16), 1024)
        R.add("rr_trig_kernel", "large/trig/%s/%s" % (arith, out_dtype), (fb, _cdiv(rows_out, rpb), rpb))


def _aligned(ldx_bytes, x_align):
    return ldx_bytes % 16 == 0 and x_align % 16 == 0


def _mfma(R, x_dtype, out_dtype, m, mpad, dpad, n, variant, ldx_bytes, x_align, env, cu, deterministic=False):
    """rr_features_mfma_launch; true when it launched."""
    if "RR_FEATURES_NO_MFMA" in env or not _aligned(ldx_bytes, x_align) or m < 1:
        return False
    g = mfma_grid(mpad, n, dpad, cu, env)
    R.add("rr_rff_features_mfma_kernel", "mfma/DMAX=%d/%s/%s" % (dpad, _pair(x_dtype, out_dtype), variant), g)
    if variant == "has_y" and deterministic:
        R.kernels.update(det_reduce(g[1] * 8, 2 * n))
        R.rows.append("mfma/deterministic")
    return True


def _mfma64(R, x_dtype, out_dtype, m, mpad, dpad, n, with_y, ldx_bytes, x_align, ldp, env, cu, deterministic=False):
    """rr_features_mfma64_launch; true when it launched."""
    osz = 4 if out_dtype == "f32" else 8
    if "RR_FEATURES_NO_MFMA64" in env or not _aligned(ldx_bytes, x_align) or m < 1 or osz * 20 * ldp >= 1 << 32:
        return False
    g = mfma64_grid(mpad, n, dpad, cu)
    R.add("rr_rff_features_mfma64_kernel", "mfma64/DMAX=%d/%s/%s" % (dpad, _pair(x_dtype, out_dtype), "has_y" if with_y else "plain"), g)
    if with_y and deterministic:
        R.kernels.update(det_reduce(g[1] * 4, 2 * n))
        R.rows.append("mfma64/deterministic")
    return True


def _valu_features(R, x_dtype, arith, mpad, dpad, n, with_y, deterministic=False):
    g = valu_rows_grid(mpad, n, 256)
    R.add("rr_rff_features_kernel", "valu_features/DMAX=%d/%s/%s/%s%s" % (dpad, x_dtype, arith, "has_y" if with_y else "plain",
                                                                      "/lds" if arith == "f64" else ""), g)
    if with_y and deterministic:
        R.kernels.update(det_reduce(g[1], 2 * n))


def prepare_route(d, env, on_device=False):
    """Which rescaling of W a fresh length scale takes (rr_basis_prepare / rr_basis_prepare_dev): (kernel or None, table row)."""
    if on_device:
        return "rr_scale_w_dev_kernel", "prepare/dev"
    if d <= 128 and "RR_PREPARE_ON_HOST" not in env:
        return "rr_scale_w_kernel", "prepare/kernel"
    return None, "prepare/host"


def feature_route(entry, compute, x_dtype, out_dtype, rows, d, n, ldx_bytes=None, x_align=0, with_y=False, want_pt=False, env=None,
                  cu=256, deterministic=False, prepare=True, on_device_ls=False, nout=1):
    """The kernels one call launches, as a Route (kernels: name -> launches; rows: the table rows it touches; grids).

    entry: "transform_dev" (rr_rff_transform_dev), "transform" / "grad" (the host entry points: rows staged into an aligned
    (chunk, dpad) buffer, one launch set per 256 MiB chunk), "gram" (rr_rff_gram_dev, its feature pass only), "put_rff" /
    "put_rff64" (FeatureMatrix / FeatureMatrix64), "put_gm" (FeatureMatrix.put_gm: two put_rff with the length scales on the
    device).  compute: "f32" | "f64" | "f32p64" of the handle.  `prepare`: the call is the first with these length scales.
    Route.error names a refusal (a float64-phase basis with misaligned rows)."""
    env = dict(env or {})
    R = Route()
    large, dpad, npad = basis_dims(d, n)
    xs = 4 if x_dtype == "f32" else 8
    if ldx_bytes is None:
        ldx_bytes = dpad * xs
    F = 2 * n
    if prepare and entry != "put_gm":
        k, row = prepare_route(d, env, on_device_ls)
        R.rows.append(row)
        if k:
            R.kernels[k] += 1
    if rows == 0:
        return R
    if entry in ("transform", "grad"):   # rr_rff_transform / rr_rff_grad: stage_alloc's chunks, each aligned with ldx = dpad
        osz = 4 if out_dtype == "f32" else 8
        out_row = F * osz * (1 if entry == "transform" else nout)
        chunk = max(1, min((256 << 20) // (dpad * xs + out_row), rows))
        for r0 in range(0, rows, chunk):
            sub = feature_route(entry + "_dev", compute, x_dtype, out_dtype, min(chunk, rows - r0), d, n, dpad * xs, 0, env=env,
                                cu=cu, prepare=False)
            R.kernels.update(sub.kernels)
            R.rows += sub.rows
            R.grids += sub.grids
        return R
    if entry in ("gm_transform", "gm_grad"):   # gm_host_call: 1 GiB staging chunks, launch_gm (rows per block 64 / 16, clamped)
        osz = 4 if out_dtype == "f32" else 8
        grad = entry == "gm_grad"
        out_row = 4 * n * (d if grad else 1)
        chunk = max(1, min((1 << 30) // (dpad * xs + out_row * osz * (2 if grad else 1)), rows))
        arith = "f64" if compute in ("f64", "f32p64") else "f32"
        for r0 in range(0, rows, chunk):
            R.add("rr_gm_grad_kernel" if grad else "rr_gm_transform_kernel", "%s/DMAX=%d/%s/%s/%s" % (entry, dpad, x_dtype, arith, out_dtype),
                  valu_rows_grid(min(chunk, rows - r0), n, 16 if grad else 64))
        return R
    arith = "f64" if compute in ("f64", "f32p64") else "f32"   # transform_dev_impl / grad_dev_impl: phase64 -> float64 arithmetic
    if entry == "transform_dev":
        ldphi = F
        if large:
            _large(R, arith, x_dtype, out_dtype, rows, rows, dpad, npad, n, False, cu)
            return R
        N = rows
        if arith == "f32":
            full = N // 32 * 32
            if full > 0 and _mfma(R, x_dtype, out_dtype, full, full, dpad, n, "plain", ldx_bytes, x_align, env, cu):
                N -= full
        else:
            full = N // 16 * 16
            if full > 0 and _mfma64(R, x_dtype, out_dtype, full, full, dpad, n, False, ldx_bytes, x_align, ldphi, env, cu):
                N -= full
        if N > 0:
            R.add("rr_rff_transform_kernel", "valu_transform/DMAX=%d/%s/%s/%s%s" % (dpad, x_dtype, arith, out_dtype,
                                                                                "/lds" if arith == "f64" else ""),
                  valu_transform_grid(N, n, cu))
        return R
    if entry == "grad_dev":
        if large:
            _large(R, arith, x_dtype, arith, rows, rows, dpad, npad, n, False, cu)
            R.add("rr_rff_grad_p_kernel", "large/grad_p/%s/%s/%s" % (x_dtype, arith, out_dtype), valu_rows_grid(rows, n, 16))
        else:
            R.add("rr_rff_grad_kernel", "valu_grad/DMAX=%d/%s/%s/%s" % (dpad, x_dtype, arith, out_dtype), valu_rows_grid(rows, n, 16))
        return R
    if entry == "gram":   # launch_gram<TX, TC>, the f32 engine, one chunk
        tc = "f32" if compute in ("f32", "f32p64") else "f64"
        KB = 32 if tc == "f32" else 16
        mpad = _cdiv(rows, KB) * KB
        ldp = _cdiv(F, 256) * 256 if tc == "f32" else _cdiv(F, 128) * 128
        if compute == "f32p64":
            if not _mfma64(R, x_dtype, "f32", rows, mpad, dpad, n, with_y, ldx_bytes, x_align, ldp, env, cu, deterministic):
                R.error = "a float64-phase basis (RR_F32P64) needs 16-byte aligned rows of X"
        elif large:
            _large(R, tc, x_dtype, tc, rows, mpad, dpad, npad, n, with_y, cu)
        elif tc == "f32":
            if not _mfma(R, x_dtype, "f32", rows, mpad, dpad, n, "has_y" if with_y else "plain", ldx_bytes, x_align, env, cu, deterministic):
                _valu_features(R, x_dtype, "f32", mpad, dpad, n, with_y, deterministic)
        elif not _mfma64(R, x_dtype, "f64", rows, mpad, dpad, n, with_y, ldx_bytes, x_align, ldp, env, cu, deterministic):
            _valu_features(R, x_dtype, "f64", mpad, dpad, n, with_y, deterministic)
        return R
    if entry in ("put_rff", "put_gm"):   # rr_features_rowmajor_f32 with m = mpad = rows
        times = 1
        if entry == "put_gm":   # two blocks, each behind its own device-side rescaling (rr_fm_put_rff_dev with a shift)
            times = 2
            R.kernels["rr_scale_w_dev_kernel"] += 2
            R.rows.append("prepare/dev")
        for _ in range(times):
            if compute == "f32p64":
                if not _mfma64(R, x_dtype, "f32", rows, rows, dpad, n, False, ldx_bytes, x_align, 256, env, cu):
                    R.error = "a float64-phase basis (RR_F32P64) needs 16-byte aligned rows of X"
            elif large:
                _large(R, "f32", x_dtype, "f32", rows, rows, dpad, npad, n, False, cu)
            elif want_pt and _mfma(R, x_dtype, "f32", rows, rows, dpad, n, "wt", ldx_bytes, x_align, env, cu):
                pass
            elif not _mfma(R, x_dtype, "f32", rows, rows, dpad, n, "plain", ldx_bytes, x_align, env, cu):
                _valu_features(R, x_dtype, "f32", rows, dpad, n, False)
        return R
    if entry == "put_rff64":   # rr_features_rowmajor_f64 with mpad = rows rounded up to 16
        mpad = _cdiv(rows, 16) * 16
        if large:
            _large(R, "f64", x_dtype, "f64", rows, mpad, dpad, npad, n, False, cu)
        elif not _mfma64(R, x_dtype, "f64", rows, mpad, dpad, n, False, ldx_bytes, x_align, 128, env, cu):
            _valu_features(R, x_dtype, "f64", mpad, dpad, n, False)
        return R
    raise ValueError(entry)


def effective_arith(entry, compute):
    """The arithmetic of the feature kernel behind an entry point: transform / grad of a float64-phase basis run wholly in
    float64 (transform_dev_impl), its Gram and its FeatureMatrix block on the float64 matrix cores with the float32 hardware
    sine / cosine (RR_F32P64 in rr_rff_features_mfma64_kernel); FeatureMatrix64 is float64 whatever the handle."""
    if entry == "put_rff64":
        return "f64"
    if compute == "f32p64":
        return "f64" if entry in ("transform", "transform_dev", "grad", "gm_transform", "gm_grad") else "f32p64"
    return compute


# Rows of the table that no public entry point reaches, with the reason (test_rff_cases_host.py: coverage).
UNREACHABLE = {
    "valu_transform grid clamp": "launch_transform's rows per block are at least N / (16 CUs), so its grid.y exceeds 65535 only "
                                 "above 4095 CUs; the clamp line is restated (valu_transform_grid) and cannot run on this chip",
    "pointer misaligned with ldx a multiple of 16 bytes through DeviceMatrix views": "a row offset of such a matrix keeps the "
                                 "16-byte alignment of the allocation; reached by a raw pointer 4 or 8 bytes into a buffer instead",
    "f32p64 VALU fallback": "launch_gram and rr_features_rowmajor_f32 refuse a float64-phase basis whose rows are misaligned or "
                            "under RR_FEATURES_NO_MFMA64 (RR_ERR_UNSUPPORTED): there is no VALU kernel with float32 sine / cosine "
                            "of a float64 phase; the refusal itself is asserted",
    "mfma64 ldp limit": "rr_features_mfma64_launch's refusal at sizeof(TO) * 20 * ldp >= 2^32 needs a leading dimension of 2^25 "
                        "doubles; restated in _mfma64, not run",
    "mfma WT with float64 output, targets or a misaligned Pt": "rr_features_rowmajor_f32 is the only caller that passes Pt: "
                        "float32 output, no targets, Pt rows of max_rows floats from the feature matrix' own aligned scratch",
}


# ---- data -------------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "label entry compute xdt odt rows d n family ard k seed with_y det want_pt ldx_extra ptr_off env big")


def case(label, entry, compute, rows, d, n, family="A", xdt=None, odt=None, ard=False, k=None, seed=0, with_y=False, det=False,
         want_pt=False, ldx_extra=0, ptr_off=0, env=(), big=False):
    xdt = xdt or ("f32" if compute == "f32" else "f64")
    odt = odt or {"gram": "f64", "put_rff": "f32", "put_gm": "f32", "put_rff64": "f64"}.get(entry, "f64" if compute == "f64" else "f32")
    k = k if k is not None else (10 if effective_arith(entry, compute) == "f32" else 12)
    return Case(label, entry, compute, xdt, odt, rows, d, n, family, ard, k, seed, with_y, det, want_pt, ldx_extra, ptr_off,
                tuple(sorted(dict(env).items())), big)


def case_route(c, cu, env=None):
    """The route of the one measured call of a case."""
    large, dpad, npad = basis_dims(c.d, c.n)
    xs = 4 if c.xdt == "f32" else 8
    e = dict(c.env)
    e.update(env or {})
    return feature_route(c.entry, c.compute, c.xdt, c.odt, c.rows, c.d, c.n, (dpad + c.ldx_extra) * xs, c.ptr_off, with_y=c.with_y,
                         want_pt=c.want_pt, env=e, cu=cu, deterministic=c.det, nout=c.d if (c.ard or c.entry == "gm_grad") else 1)


_DATA = {}


def lenscales(d, ard, seed, family):
    if family == "A":   # powers of two: W (inv2pi / l) is an exact scaling of W inv2pi
        if ard:
            return 2.0 ** np.random.RandomState(seed + 11).randint(-1, 3, d)
        return np.array([(0.5, 1.0, 4.0)[seed % 3]])
    return np.linspace(0.6, 1.7, d) if ard else np.array([1.3])


def dyadic_data(rows, d, n, k, ard, seed, exact_below):
    """Family A.  exact_below: the float32 limit 2^24 on sum |x Q|, or 64 * 2^k for float64 arithmetic (64 revolutions)."""
    rs = np.random.RandomState(1000 * seed + 7 * d + n)
    ls = lenscales(d, ard, seed, "A")
    qmax = int(min(max((exact_below - 1) // (8 * d), 1), 1 << 20))
    Q = 2 * rs.randint(-(qmax // 2) - 1, (qmax + 1) // 2, (d, n)).astype(np.int64) + 1   # odd: never zero, never a whole turn
    Q = np.clip(Q, -qmax, qmax)
    Q[Q == 0] = 1
    X = rs.randint(-8, 9, (rows, d)).astype(np.int64)
    X[rs.rand(rows, d) < 0.25] = 0
    li = np.broadcast_to(ls, (d,))
    W = TWO_PI * (Q * li[:, None] / 2.0 ** k)          # Q l / 2^k is exact; one rounding by the product with 2 pi
    Ws64 = W * (INV2PI / li)[:, None]                   # the library's own two float64 operations
    want = Q / 2.0 ** k
    assert np.array_equal(Ws64.astype(np.float32).astype(np.float64), want), "float32(Ws) is not Q / 2^k"
    # two float64 roundings (the product with 2 pi above, the library's product with inv2pi / l) and the literals' own error:
    # asserted to stay within two units, the "+ 2" of the float64 phase term (phase_term)
    assert np.all(np.abs(Ws64 - want) <= 2 * U64 * np.abs(want)), float((np.abs(Ws64 - want) / np.abs(want)).max())
    aS = np.abs(X) @ np.abs(Q)
    assert int(aS.max()) < exact_below, (int(aS.max()), exact_below)
    S = X @ Q
    half = 1 << (k - 1)
    r = ((S + half) % (1 << k)) - half                  # exact: the phase modulo one revolution, in [-1/2, 1/2)
    ang = TWO_PI_L * (r.astype(np.longdouble) / np.longdouble(2 ** k))
    return SimpleNamespace(family="A", X=X.astype(np.float64), W=W, ls=ls, Q=Q, k=k, S=S, want=np.concatenate((np.cos(ang), np.sin(ang)), axis=1),
                           phase=S / 2.0 ** k, A=aS / 2.0 ** k, Ws64=Ws64)


def real_data(rows, d, n, ard, seed):
    """Family B: Gaussian x (float32-representable, so that float32 and float64 inputs carry the same values), Gaussian W
    scaled so that A = sum_i |x_i W_if / (2 pi l_i)| is at most two revolutions."""
    rs = np.random.RandomState(2000 * seed + 7 * d + n + 1)
    ls = lenscales(d, ard, seed, "B")
    X = rs.randn(rows, d).astype(np.float32).astype(np.float64)
    W = rs.randn(d, n)
    li = np.broadcast_to(ls, (d,))
    A = np.abs(X) @ np.abs(W / (TWO_PI * li)[:, None])
    W = W * (1.999 / A.max())
    Wl = W.astype(np.longdouble) / (TWO_PI_L * li.astype(np.longdouble))[:, None]
    ph = X.astype(np.longdouble) @ Wl
    A = (np.abs(X).astype(np.longdouble) @ np.abs(Wl)).astype(np.float64)
    assert A.max() <= 2.0
    f = ph - np.rint(ph)
    return SimpleNamespace(family="B", X=X, W=W, ls=ls, want=np.concatenate((np.cos(TWO_PI_L * f), np.sin(TWO_PI_L * f)), axis=1),
                           phase=ph.astype(np.float64), A=A, Ws64=W * (INV2PI / li)[:, None])


def case_data(c):
    """The data set of a case (cached, read-only): X (float64 values; the case's xdt says what is uploaded), W, ls, the
    reference `want` = [cos | sin] at unit amplitude in long double, the phase and A in revolutions, and integer targets y."""
    arith = effective_arith(c.entry, c.compute)
    exact_below = (1 << 24) if arith == "f32" else 64 << c.k
    if c.entry in ("gm_transform", "gm_grad"):
        exact_below //= 2   # the other half is the mean's (gm_data)
    key =(c.family, c.rows, c.d, c.n, c.k, c.ard, c.seed, exact_below if c.family == "A" else 0)
    if key not in _DATA:
        if len(_DATA) > 48:
            _DATA.clear()
        D = dyadic_data(c.rows, c.d, c.n, c.k, c.ard, c.seed, exact_below) if c.family == "A" else real_data(c.rows, c.d, c.n, c.ard, c.seed)
        D.y = np.random.RandomState(c.rows + 3).randint(-3, 4, c.rows).astype(np.float64)
        for a in (D.X, D.W, D.want, D.phase, D.A, D.y):
            a.setflags(write=False)
        _DATA[key] = D
    return _DATA[key]


def lenscale_arg(D, c):
    return D.ls if c.ard else float(D.ls[0])


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def gamma(m, u):
    return m * u / (1 - m * u)


def phase_term(arith, family, d, A, extra=0):
    """Bound on the error of the phase (revolutions) times 2 pi: |d cos|, |d sin| <= 2 pi |d phase|.

    float32, family A: nothing -- Ws and every partial sum are exact (dyadic_data's assertions).
    float32, family B: gamma(d + 2) A with u = 2^-24: the cast of Ws to float32 (rr_scale_w_kernel: `vf = (float) v`), the
        cast of a float64 x on load (project_row: `(TC) xr[i]`, the matrix-core kernel: `a[t] = (float) src[t]`, rr_xt_kernel)
        and d roundings of the fused multiply-adds (project_row) or of the matrix cores' products and sums, in any order.
    float64 and f32p64: the same with u = 2^-53; there the two roundings of Ws = W (inv2pi / l) take the place of the casts.
        Family A keeps the first-order form (d + 2) u A: its data's own assertion (Ws64 within 2 u of Q / 2^k) and d fused
        multiply-adds.
    extra: further roundings of a value of at most A (the spectral-mixture kernels' `z + mx`: one)."""
    m = d + 2 + extra
    if arith == "f32":
        return 0.0 * A if family == "A" else TWO_PI * gamma(m, U32) * A
    return TWO_PI * (m * U64 if family == "A" else gamma(m, U64)) * A


def trig_term(arith, odt):
    """Bound on [cos | sin] sqrt(n) at an exactly known phase.

    float32 (sincos_rev(float): t - rintf(t) is exact, then v_sin_f32 / v_cos_f32; `c * scale` with scale = (float)(1 / sqrt n)):
        PHI_F32_BOUND = 2 SINCOS_F32_MAX_ERR + 2^-23; a float64 output widens the float32 product without another rounding.
    float64 (rr_sincos_rev_f64, `cv * scale`): PHI_F64_BOUND, plus 2^-24 where the result is stored as float32.
    f32p64 (rr_rff_features_mfma64_kernel, ES == 4): `fr = (float)(acc - rint(acc))` rounds a value of at most 1/2 to float32,
        half an ulp of [1/4, 1/2) = 2^-26 revolutions; then the float32 instructions and `cf * fs`, fs = (float) scale, as in
        float32 -- the product's rounding is the output's 2^-24."""
    if arith == "f32":
        return PHI_F32_BOUND
    if arith == "f64":
        return PHI_F64_BOUND + (U32 if odt == "f32" else 0.0)
    return TWO_PI * 2.0 ** -26 + PHI_F32_BOUND


def phi_bound(arith, odt, family, d, A, n):
    """Per-element bound on |Phi sqrt(n) - want|, both blocks (tiled); + 1e-36 sqrt(n) for flushed subnormals (family B)."""
    b = phase_term(arith, family, d, A) + trig_term(arith, odt)
    if family == "B":
        b = b + 1e-36 * np.sqrt(n)
    return np.tile(b, (1, 2))


GRAD_ROUNDINGS = {
    # rr_rff_grad_kernel: dz = -(TC) xr[i] * w[i] * gfac[i] * scale, then -s * dz / c * dz: four multiplies; operands: the cast of
    # x, of Ws, of gfac = 2 pi / l and of scale = 1 / sqrt n to float32: eight roundings
    ("f32", False): 8,
    # rr_rff_grad_p_kernel: dz = -(TC) xr[i] * Ws * gfac[i] (two multiplies), s * dz (one); P = c * scale as stored (the product and
    # the cast of scale); the casts of x, Ws and gfac: eight again
    ("f32", True): 8,
    # float64: Ws = W * (inv2pi / l) (the literal, the quotient, the product), gfac = twopi / l (literal, quotient), scale
    # (square root, quotient), four multiplies: eleven, one more for the literal of the reference's own 2 pi
    ("f64", False): 12, ("f64", True): 12}


def grad_reference(D, c):
    """(want, |dz|): dPhi/dl_i = [-sin(z) dz_i, cos(z) dz_i] at unit amplitude, dz_i = -x_i W_if / l_i^2; (rows, 2n, nout), nout
    = d for ARD length scales and 1 -- dimension 0 only, the reference's isotropic quirk -- otherwise."""
    n = c.n
    nout = c.d if c.ard else 1
    li = np.broadcast_to(D.ls, (c.d,)).astype(np.longdouble)
    dz = -(D.X[:, None, :nout].astype(np.longdouble) * D.W.T[None, :, :nout].astype(np.longdouble)) / (li[:nout] ** 2)   # (rows, n, nout)
    cosv, sinv = D.want[:, :n, None], D.want[:, n:, None]
    want = np.concatenate((-sinv * dz, cosv * dz), axis=1)
    return want, np.abs(np.concatenate((dz, dz), axis=1)).astype(np.float64)


def grad_bound(arith, odt, family, d, A, adz, large):
    """Per-entry bound on |dPhi sqrt(n) - want|, relative to the entry's own |dz_i|: the sine / cosine at the computed phase is
    off by at most the phase term plus the instruction's error (2 SINCOS_F32_MAX_ERR in float32, PHI_F64_BOUND in float64, no
    scale multiply in it: that is one of the counted roundings), every counted rounding moves a product of magnitude at most
    |dz| by u, a float32 store of float64 arithmetic by 2^-24 more; 1e-36 for flushed subnormals."""
    u = U32 if arith == "f32" else U64
    trig = 2 * SINCOS_F32_MAX_ERR if arith == "f32" else PHI_F64_BOUND
    t = (phase_term(arith, family, d, A) + trig)[:, :, None]
    g = gamma(GRAD_ROUNDINGS[(arith, large)], u)
    rel = np.concatenate((t, t), axis=1) * (1 + g) + g
    if arith == "f64" and odt == "f32":
        rel = rel + U32
    return rel * adz + 1e-36


def gm_data(c):
    """case_data plus a mean for the spectral-mixture kernels (phases z +- x . mean / (2 pi)): family A mean = 2 pi M / 2^k with
    integer M (mu = mean inv2pi rounds to M / 2^k exactly in float32, asserted; sum |x| (|Q| + |M|) below the exact limit),
    family B Gaussian, at most one revolution of A_m = sum |x_i mean_i / (2 pi)|.  want4: [cos, sin](z + m), [cos, sin](z - m)."""
    D = case_data(c)
    if getattr(D, "mean", None) is not None:
        return D
    rs = np.random.RandomState(c.seed + 5)
    X = D.X
    if c.family == "A":
        qmax = int(np.abs(D.Q).max())
        M = rs.randint(-qmax, qmax + 1, c.d).astype(np.int64)
        mean = TWO_PI * (M / 2.0 ** c.k)
        mu = mean * INV2PI
        assert np.array_equal(mu.astype(np.float32).astype(np.float64), M / 2.0 ** c.k)
        assert np.all(np.abs(mu - M / 2.0 ** c.k) <= 2 * U64 * np.abs(M / 2.0 ** c.k))
        Xi = X.astype(np.int64)
        SM = Xi @ M
        aM = np.abs(Xi) @ np.abs(M)
        limit = (1 << 24) if effective_arith(c.entry, c.compute) == "f32" else 64 << c.k
        assert int((np.abs(Xi) @ np.abs(D.Q)).max() + aM.max()) < limit
        half = 1 << (c.k - 1)
        blocks = []
        for sgn in (1, -1):
            r = ((D.S + sgn * SM[:, None] + half) % (1 << c.k)) - half
            ang = TWO_PI_L * (r.astype(np.longdouble) / np.longdouble(2 ** c.k))
            blocks += [np.cos(ang), np.sin(ang)]
        Am = aM / 2.0 ** c.k
    else:
        mean = rs.randn(c.d)
        Am = np.abs(X) @ np.abs(mean / TWO_PI)
        mean = mean * (0.999 / Am.max())
        ml = mean.astype(np.longdouble) / TWO_PI_L
        mx = (X.astype(np.longdouble) @ ml)[:, None]
        Am = (np.abs(X).astype(np.longdouble) @ np.abs(ml)).astype(np.float64)
        li = np.broadcast_to(D.ls, (c.d,)).astype(np.longdouble)
        z = X.astype(np.longdouble) @ (D.W.astype(np.longdouble) / (TWO_PI_L * li)[:, None])
        blocks = []
        for sgn in (1, -1):
            ph = z + sgn * mx
            f = ph - np.rint(ph)
            blocks += [np.cos(TWO_PI_L * f), np.sin(TWO_PI_L * f)]
    D.mean, D.want4, D.Agm = mean, np.concatenate(blocks, axis=1), D.A + Am[:, None]
    for a in (D.mean, D.want4, D.Agm):
        a.setflags(write=False)
    return D


def gm_phi_bound(arith, odt, family, d, Agm, n):
    """phi_bound for the four blocks at amplitude sqrt(2 n): the phase term over A_z + A_m with one more rounding, the add of
    `sincos_rev(z + mx, ...)`; z and mx are fused multiply-add chains like the projection (rr_gm_transform_kernel)."""
    b = phase_term(arith, family, d, Agm, extra=1) + trig_term(arith, odt)
    if family == "B":
        b = b + 1e-36 * np.sqrt(2 * n)
    return np.tile(b, (1, 4))


def gm_grad_reference(D, c):
    """(dmean, |x|, dlen, |dz|) at unit amplitude, each (rows, 4n, d): dmean_i = x_i [-sin+, cos+, sin-, -cos-],
    dlen_i = dz_i [-sin+, cos+, -sin-, cos-]."""
    n = c.n
    li = np.broadcast_to(D.ls, (c.d,)).astype(np.longdouble)
    x = D.X[:, None, :].astype(np.longdouble)
    dz = -(x * D.W.T[None].astype(np.longdouble)) / (li ** 2)
    cp, sp, cm, sm = (D.want4[:, i * n:(i + 1) * n, None] for i in range(4))
    dmean = np.concatenate((-sp * x, cp * x, sm * x, -cm * x), axis=1)
    dlen = np.concatenate((-sp * dz, cp * dz, -sm * dz, cm * dz), axis=1)
    ax = np.abs(np.broadcast_to(x, dz.shape))
    return dmean, np.tile(ax, (1, 4, 1)).astype(np.float64), dlen, np.tile(np.abs(dz), (1, 4, 1)).astype(np.float64)


# rr_gm_grad_kernel: xi = (TC) xr[i] * scale, then -sp * xi: the casts of x and of scale = 1 / sqrt(2 n), two multiplies; float64:
# the square root and the quotient of scale, two multiplies.  dlen: as rr_rff_grad_kernel.
GM_DMEAN_ROUNDINGS = {"f32": 4, "f64": 4}


def gm_grad_bound(arith, odt, family, d, Agm, mag, roundings):
    u = U32 if arith == "f32" else U64
    trig = 2 * SINCOS_F32_MAX_ERR if arith == "f32" else PHI_F64_BOUND
    t = np.tile(phase_term(arith, family, d, Agm, extra=1) + trig, (1, 4))[:, :, None]
    g = gamma(roundings, u)
    rel = t * (1 + g) + g
    if arith == "f64" and odt == "f32":
        rel = rel + U32
    return rel * mag + 1e-36


def bty_bound(arith, bound_phi, want, y, rows):
    """Phi^T y sqrt(n) against sum_r y_r want_rf: the per-element bounds summed with |y_r|, plus rows u sum_r |y_r Phi_rf| for
    the in-kernel accumulation (fmaf(cv, yv, bc) in float32; fma in float64 for the float64 and f32p64 kernels), plus the
    float64 atomics across workgroups, rows 2^-53 of the same sum."""
    u = U32 if arith == "f32" else U64
    ay = np.abs(y)[:, None]
    s = (ay * np.abs(want).astype(np.float64)).sum(axis=0)
    return (ay * bound_phi).sum(axis=0) + rows * (u + U64) * (s + (ay * bound_phi).sum(axis=0))


def report(label, route, got_amp, want, bound, phase, n):
    """(ratio, message): the worst element's row, frequency, block, phase and ratio to its bound."""
    err = np.abs(got_amp - want).astype(np.float64)
    ratio = err / bound
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    r, col = int(i[0]), int(i[1])
    f, blk = col % n, ("cos", "sin")[(col // n) % 2]
    msg = ("%s [%s]: worst element row %d frequency %d block %s%s, phase %.6f rev, |error| %.3e, bound %.3e, ratio %.3f; %d of %d beyond"
           % (label, "+".join(sorted(set(route))) if route else "-", r, f, blk, (" dim %d" % i[2]) if len(i) > 2 else "",
              float(phase[r, f]), float(err[i]), float(np.broadcast_to(bound, err.shape)[i]), float(ratio[i]), int((ratio > 1).sum()), err.size))
    return float(ratio[i]), msg


# ---- float32 / float64 emulation of the projection (test_rff_cases_host.py: the bound admits correct code and rejects wrong) ----
def _sum_order(P, order):
    """Sum P (rows, d, n) over axis 1 in P's own precision, rounding after every add."""
    d = P.shape[1]
    if order == "ascending":
        idx = list(range(d))
    elif order == "even_odd":
        idx = list(range(0, d, 2)) + list(range(1, d, 2))
    else:   # pairwise
        parts = [P[:, i] for i in range(d)]
        while len(parts) > 1:
            parts = [parts[i] + parts[i + 1] if i + 1 < len(parts) else parts[i] for i in range(0, len(parts), 2)]
        return parts[0]
    acc = np.zeros((P.shape[0], P.shape[2]), dtype=P.dtype)
    for i in idx:
        acc = acc + P[:, i]
    return acc


def round_mantissa(x, bits):
    """x rounded to `bits` explicit mantissa bits."""
    m, e = np.frexp(x)
    return np.ldexp(np.rint(m * 2.0 ** (bits + 1)) / 2.0 ** (bits + 1), e)


MUTANTS = ("drop_last_dim", "x_10bit", "sin_sign", "swap_blocks", "inv2pi_1e-12")
INV2PI_TRUNC = 0.159154943091   # the literal cut after twelve digits: 5.6e-12 relative


def emulate(D, arith, order="ascending", mutant=None):
    """[cos | sin] at unit amplitude from a NumPy emulation of the kernels' projection in `arith`: Ws and x rounded to the
    type, a rounding after every product and every add in the given order, float64 sine / cosine of the exactly reduced phase.
    Returns (values, mask of the elements a mutant touches)."""
    T = NP[arith]
    X = D.X
    li = np.broadcast_to(D.ls, (X.shape[1],))
    Ws = D.W * ((INV2PI_TRUNC if mutant == "inv2pi_1e-12" else INV2PI) / li)[:, None]
    n = Ws.shape[1]
    if mutant == "drop_last_dim":
        X = X.copy()
        X[:, -1] = 0
    if mutant == "x_10bit":
        X = round_mantissa(X, 10)
    P = X.astype(T)[:, :, None] * Ws.astype(T)[None]
    t = _sum_order(P, order).astype(np.float64)
    f = t - np.rint(t)
    out = np.concatenate((np.cos(TWO_PI * f), np.sin(TWO_PI * f)), axis=1)
    mask = np.ones(out.shape, dtype=bool)
    if mutant == "sin_sign":
        out[:, n:] = -out[:, n:]
        mask[:, :n] = False
    if mutant == "swap_blocks":   # the first block of 32 frequencies: column f <-> column n + f
        w = min(32, n)
        out[:, :w], out[:, n:n + w] = out[:, n:n + w].copy(), out[:, :w].copy()
        mask[:] = False
        mask[:, :w] = mask[:, n:n + w] = True
    return out, mask


# ---- the case lists -----------------------------------------------------------------------------------------------------------
ROWS_EDGE = (1, 15, 16, 17, 31, 32, 33, 63)
N_EDGE = (1, 15, 17, 31, 33, 129, 257)
D_EDGE = (1, 7, 8, 9, 16, 17, 33, 65, 128)


def transform_cases():
    """rr_rff_transform_dev into a sentinel-filled buffer: the row edges of both tile sizes, ragged frequency blocks, every DMAX,
    every (x, compute, out) type, both families."""
    out = []
    for compute in ("f32", "f64"):
        for rows in ROWS_EDGE:
            out.append(case("t/%s/rows=%d" % (compute, rows), "transform_dev", compute, rows, 9, 33, seed=rows))
        for n in N_EDGE:
            out.append(case("t/%s/n=%d" % (compute, n), "transform_dev", compute, 49, 7, n, seed=n, ard=True))
        for d in D_EDGE:
            out.append(case("t/%s/d=%d" % (compute, d), "transform_dev", compute, 33 + 16, d, 40, seed=d, ard=d % 2 == 1))
            out.append(case("tB/%s/d=%d" % (compute, d), "transform_dev", compute, 33 + 16, d, 40, family="B", seed=d, ard=d % 2 == 0))
    # every (x type, out type) pair on each kernel family, at every DMAX of the matrix-core kernels
    for compute in ("f32", "f64", "f32p64"):
        for xdt in ("f32", "f64"):
            for odt in ("f32", "f64"):
                for d in (8, 16, 32, 64, 128):
                    fam = "B" if (d // 8 + (xdt == "f64") + (odt == "f64")) % 2 else "A"
                    out.append(case("t/%s/%s->%s/d=%d" % (compute, xdt, odt, d), "transform_dev", compute, 32 + 16 + 5, d, 35, family=fam,
                                    xdt=xdt, odt=odt, seed=d + 1, ard=True))
    # the tiles-per-workgroup walk of rr_features_mfma_launch at 256 CUs: 32 t + r rows, few column groups
    # (tpb = 4, 8, 16, 32 there; 64 of its own accord takes 2^16 wave tiles, 0.5 GB of features: forced by RR_FEAT_TPB = 64, which
    # the launcher reads per call, on 70 tiles -- a workgroup of 16 tiles per wave and a partial one)
    for t in (2, 3000, 9000, 40000):
        out.append(case("t/f32/tpb/%dx32+5" % t, "transform_dev", "f32", 32 * t + 5, 8, 8, seed=t % 7, big=t > 10000))
    out.append(case("t/f32/tpb/RR_FEAT_TPB=64", "transform_dev", "f32", 32 * 70 + 5, 8, 8, seed=5, env={"RR_FEAT_TPB": "64"}))
    out.append(case("t/f32/tpb/RR_FEAT_TPB=3", "transform_dev", "f32", 32 * 70 + 5, 40, 129, seed=5, env={"RR_FEAT_TPB": "3"}))
    for t in (3, 20000, 40000):   # rr_features_mfma64_launch: tpb = 4, 8, 16
        out.append(case("t/f64/tpb/%dx16+5" % t, "transform_dev", "f64", 16 * t + 5, 8, 8, seed=t % 5, big=t > 10000))
    return out


def align_cases():
    """Rows whose stride or address is not a multiple of 16 bytes: the VALU kernels for the whole call."""
    out = []
    for compute in ("f32", "f64"):
        for d in (5, 16, 100):
            out.append(case("t/%s/ldx+1/d=%d" % (compute, d), "transform_dev", compute, 49, d, 33, ldx_extra=1, seed=d))
            out.append(case("tB/%s/ldx+1/d=%d" % (compute, d), "transform_dev", compute, 49, d, 33, ldx_extra=1, family="B", seed=d, ard=True))
        out.append(case("t/%s/ptr+8/d=16" % compute, "transform_dev", compute, 49, 16, 33, ptr_off=8, ldx_extra=4, seed=3))
        out.append(case("gram/%s/ldx+1" % compute, "gram", compute, 70, 9, 40, ldx_extra=1, with_y=True, seed=4))
        out.append(case("gram/%s/ldx+1/no y" % compute, "gram", compute, 70, 20, 40, ldx_extra=1, seed=5, family="B"))
    out.append(case("put/f32/ldx+1", "put_rff", "f32", 70, 40, 33, ldx_extra=1, seed=6))
    out.append(case("put/f32/f64 x/ldx+1", "put_rff", "f32", 70, 70, 33, ldx_extra=1, xdt="f64", seed=6, family="B"))
    out.append(case("put64/f64/ldx+1", "put_rff64", "f64", 70, 9, 33, ldx_extra=1, seed=7))
    out.append(case("put64/f64/f32 x/ldx+1", "put_rff64", "f64", 70, 128, 33, ldx_extra=1, xdt="f32", seed=7, family="B"))
    return out


def grad_cases():
    out = []
    for compute in ("f32", "f64"):
        for d in D_EDGE:
            out.append(case("g/%s/d=%d" % (compute, d), "grad", compute, 19, d, 33, seed=d, ard=d != 9))
            if d in (1, 8, 33, 128):
                out.append(case("gB/%s/d=%d" % (compute, d), "grad", compute, 19, d, 17, family="B", seed=d, ard=d != 8))
        out.append(case("g/%s/n=257" % compute, "grad", compute, 17, 7, 257, seed=2, ard=True))
        for xdt in ("f32", "f64"):
            for odt in ("f32", "f64"):
                out.append(case("g/%s/%s->%s" % (compute, xdt, odt), "grad", compute, 17, 7, 31, seed=2, ard=xdt == odt, odt=odt, xdt=xdt))
    out.append(case("g/f32p64", "grad", "f32p64", 17, 7, 31, seed=2, ard=True))
    return out


def large_cases():
    """Xdim > 128: the three shapes of large_features, through every entry point that reaches them."""
    out = []
    for d in (129, 200):
        for compute, xdt, odt in (("f32", "f32", "f32"), ("f32", "f64", "f64"), ("f32", "f64", "f32"), ("f32", "f32", "f64"),
                                   ("f64", "f64", "f64"), ("f64", "f32", "f32")):
            out.append(case("L/t/%s/%s->%s/d=%d" % (compute, xdt, odt, d), "transform_dev", compute, 33, d, 17, xdt=xdt, odt=odt, seed=d))
            out.append(case("LB/t/%s/%s->%s/d=%d" % (compute, xdt, odt, d), "transform_dev", compute, 33, d, 17, xdt=xdt, odt=odt, seed=d,
                            family="B", ard=True))
        for compute in ("f32", "f64"):
            out.append(case("L/g/%s/d=%d" % (compute, d), "grad", compute, 9, d, 17, seed=d, ard=d == 200))
            out.append(case("L/gram/%s/d=%d" % (compute, d), "gram", compute, 70, d, 17, seed=d, with_y=True))
        out.append(case("L/put/f32/d=%d" % d, "put_rff", "f32", 70, d, 17, seed=d))
        out.append(case("L/put64/f64/d=%d" % d, "put_rff64", "f64", 70, d, 17, seed=d))
    out.append(case("L/t/f32/n=257", "transform_dev", "f32", 300, 129, 257, seed=1))
    # the sub-chunk seam, cheaply: RR_LG_ROWS + 1 rows at four frequencies
    out.append(case("L/t/f32/seam", "transform_dev", "f32", RR_LG_ROWS + 1, 129, 4, seed=2, big=True))
    out.append(case("L/t/f32->f64/seam", "transform_dev", "f32", RR_LG_ROWS + 1, 129, 4, seed=2, odt="f64", big=True))
    out.append(case("L/t/f64/seam", "transform_dev", "f64", RR_LG_ROWS + 1, 129, 4, seed=2, big=True))
    return out


def gram_cases():
    """The feature pass of rr_rff_gram_dev: Phi^T y from the pass (HAS_Y; plain and deterministic), every DMAX."""
    out = []
    for compute in ("f32", "f64", "f32p64"):
        for d in (8, 16, 32, 64, 128):
            for xdt in ("f32", "f64"):
                fam = "B" if (d // 8 + (xdt == "f64")) % 2 else "A"
                out.append(case("gram/%s/%s x/d=%d" % (compute, xdt, d), "gram", compute, 32 * 3 + 17, d, 40, xdt=xdt, with_y=True,
                                seed=d, family=fam, ard=True))
        out.append(case("gram/%s/det" % compute, "gram", compute, 32 * 9 + 1, 9, 33, with_y=True, det=True, seed=8))
        out.append(case("gram/%s/no y" % compute, "gram", compute, 32 * 3 + 17, 9, 33, seed=8))
        out.append(case("gram/%s/n=129" % compute, "gram", compute, 63, 7, 129, with_y=True, seed=9))
    return out


def featmat_cases():
    """FeatureMatrix / FeatureMatrix64 blocks: plain, with the feature-major second output (WT), float64 phases, Xdim edges."""
    out = []
    for d in (8, 16, 32, 64, 128):
        for xdt in ("f32", "f64"):
            out.append(case("put/f32/%s x/d=%d" % (xdt, d), "put_rff", "f32", 70, d, 40, xdt=xdt, seed=d, ard=True))
            out.append(case("put/f32/%s x/d=%d/wt" % (xdt, d), "put_rff", "f32", 70, d, 40, xdt=xdt, seed=d, ard=True, want_pt=True,
                            family="B" if xdt == "f64" else "A"))
            out.append(case("put/f32p64/%s x/d=%d" % (xdt, d), "put_rff", "f32p64", 70, d, 40, xdt=xdt, seed=d,
                            family="B" if xdt == "f32" else "A"))
            out.append(case("put64/f64/%s x/d=%d" % (xdt, d), "put_rff64", "f64", 70, d, 40, xdt=xdt, seed=d,
                            family="B" if xdt == "f32" else "A"))
    out.append(case("put64/f32 handle", "put_rff64", "f32", 33, 9, 33, seed=1))
    out.append(case("put/gm", "put_gm", "f32", 70, 9, 33, seed=1, ard=True))
    return out


def gm_cases():
    """rr_gm_transform_kernel / rr_gm_grad_kernel through RffHandle.gm_transform / gm_grad: every DMAX, both families."""
    out = []
    for compute in ("f32", "f64"):
        for d in D_EDGE:
            out.append(case("gm/t/%s/d=%d" % (compute, d), "gm_transform", compute, 70, d, 33, seed=d, ard=d % 2 == 0, odt=compute))
            if d in (1, 8, 17, 128):
                out.append(case("gmB/t/%s/d=%d" % (compute, d), "gm_transform", compute, 70, d, 33, family="B", seed=d, ard=True, odt="f64",
                                xdt="f64"))
        for d in (1, 7, 9, 17, 33, 65, 128):
            out.append(case("gm/g/%s/d=%d" % (compute, d), "gm_grad", compute, 19, d, 17, seed=d, ard=True, odt="f64"))
        out.append(case("gmB/g/%s/d=20" % compute, "gm_grad", compute, 19, 20, 17, family="B", seed=2, ard=True, odt="f64"))
        out.append(case("gm/t/%s/n=257" % compute, "gm_transform", compute, 65, 7, 257, seed=1, odt="f32", xdt="f32"))
    return out


def host_cases():
    """The host entry points (staged rows): transform of a float64-phase basis, and one case per arithmetic."""
    return [case("h/t/f32", "transform", "f32", 49, 9, 33, seed=1, odt="f64"),
            case("h/t/f64", "transform", "f64", 49, 9, 33, seed=1),
            case("h/t/f32p64", "transform", "f32p64", 49, 9, 33, seed=1, odt="f64"),
            case("h/tB/f32p64", "transform", "f32p64", 49, 20, 33, seed=1, odt="f64", family="B", ard=True)]


# grid clamps (references are O(N)); the first in the default process, the other two in the RR_FEATURES_NO_MFMA child
CLAMP_MFMA = case("clamp/mfma/RR_FEAT_TPB=1", "transform_dev", "f32", 32 * 65536 + 32, 8, 1, seed=3, env={"RR_FEAT_TPB": "1"}, big=True)
CLAMP_VALU_T = case("clamp/valu/transform", "transform_dev", "f32", 16 * 65535 + 17, 8, 1, seed=4, env={"RR_FEATURES_NO_MFMA": "1"}, big=True)
CLAMP_VALU_G = case("clamp/valu/grad", "grad", "f32", 16 * 65535 + 17, 8, 1, seed=4, env={"RR_FEATURES_NO_MFMA": "1"}, big=True)

SWITCHES = ("RR_FEATURES_NO_MFMA", "RR_FEATURES_NO_MFMA64", "RR_PREPARE_ON_HOST")


def switch_cases(switch):
    """What a child process started with one of the process-start switches runs."""
    env = {switch: "1"}
    if switch == "RR_FEATURES_NO_MFMA":
        out = [case("noMFMA/t/d=%d" % d, "transform_dev", "f32", 70, d, 40, seed=d, env=env, family="B" if d in (16, 64) else "A",
                    xdt="f64" if d == 32 else "f32", odt="f64" if d == 64 else "f32") for d in (8, 16, 32, 64, 128)]
        out += [case("noMFMA/gram/d=%d" % d, "gram", "f32", 70, d, 40, seed=d, env=env, with_y=True, xdt="f64" if d == 16 else "f32")
                for d in (8, 16, 32, 64, 128)]
        out += [case("noMFMA/gram/det", "gram", "f32", 300, 9, 33, seed=1, env=env, with_y=True, det=True),
                case("noMFMA/put", "put_rff", "f32", 70, 9, 33, seed=1, env=env), CLAMP_VALU_T, CLAMP_VALU_G]
        return out
    if switch == "RR_FEATURES_NO_MFMA64":
        out = [case("noMFMA64/t/d=%d" % d, "transform_dev", "f64", 70, d, 40, seed=d, env=env, family="B" if d in (16, 64) else "A",
                    xdt="f32" if d == 32 else "f64", odt="f32" if d == 64 else "f64") for d in (8, 16, 32, 64, 128)]
        out += [case("noMFMA64/gram/d=%d" % d, "gram", "f64", 70, d, 40, seed=d, env=env, with_y=True, xdt="f32" if d == 16 else "f64")
                for d in (8, 16, 32, 64, 128)]
        out += [case("noMFMA64/gram/det", "gram", "f64", 300, 9, 33, seed=1, env=env, with_y=True, det=True),
                case("noMFMA64/put64", "put_rff64", "f64", 70, 9, 33, seed=1, env=env)]
        return out
    return [case("hostprep/t/%s" % cp, "transform_dev", cp, 49, 9, 33, seed=1, env=env, ard=ard) for cp in ("f32", "f64") for ard in (False, True)]


PREPARE_IDENTITY = case("prepare/identity", "transform_dev", "f32", 49, 9, 64, seed=1, ard=True)   # 1 / sqrt(64) = 1 / sqrt(2 * 32)


def default_cases():
    return transform_cases() + align_cases() + grad_cases() + large_cases() + gram_cases() + featmat_cases() + gm_cases() + host_cases() + [CLAMP_MFMA]


def all_cases():
    return default_cases() + [c for s in SWITCHES for c in switch_cases(s)]


def census_cases():
    """One call per case under the bounds-checking build: everything but the cases of hundreds of megabytes."""
    return [c for c in default_cases() if not c.big]
