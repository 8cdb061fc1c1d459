"""Every instance of the FastFood chain kernels (rr_fastfood.hip) against exact references.

Up to the final multiply by S the chain is +-1 signs, integer sums, a gather and a product with G: on integer data every
intermediate is exact in float32 below 2^24 (float64: 2^53) whatever order the butterflies run in.  `int_chain` computes it
in int64 with an explicit +-1 Hadamard matrix, together with the same chain over absolute values, which bounds every
intermediate; each case asserts its own bound.  With that

* VX (PHI = false) is ONE rounded multiply away from the integers: compared bit for bit where d2^-1.5 is a power of two,
  to one ulp where the library's pow() may round differently from Python's;
* Phi is taken at phases that are exact multiples of 1/16 revolution (S = 2 pi 2^-4 / d2^-1.5), so a float32 phase of
  hundreds of revolutions must be reduced exactly, and what remains is the error of the sine / cosine alone;
  (on gfx950 the sine / cosine instructions reduce arguments of this size exactly themselves -- removing the kernel's own
  t - rint(t) changes no value at phases up to 1004 revolutions, docs/KERNELS.md 3.7 -- so on this chip these cases hold
  the reduction only together with the instruction's);
* real-valued data is held element by element to the forward error bound of the chain, ((1 + u)^(2 log2 d2 + 4) - 1) A,
  A being the chain over absolute values -- not to a fraction of the largest element.

`instance` restates ff_launch's choice of kernel family, register count and VEC / FULL variant; the cases reach every
reachable instance (checked on the CPU), buffers of the device-resident calls are prefilled with a sentinel bit pattern so
that a store outside the written block shows, and the bounds-checking build counts launches per instance
(tests/test_debug_builds.py runs `census`)."""
import ctypes
import os
import subprocess
import sys
from collections import namedtuple
from types import SimpleNamespace

import numpy as np
import pytest

import revrand_oracle as orc
from conftest import ROOT

INV2PI = 0.15915494309189533576888  # the library's literal (rr_fastfood_create, ff_prepare_mean)
TWO_PI_L = 2 * np.arccos(np.longdouble(-1))
U = {"f32": 2.0 ** -24, "f64": 2.0 ** -53}
NP = {"f32": np.float32, "f64": np.float64}
EXACT = {"f32": 1 << 24, "f64": 1 << 53}
OLD = os.environ.get("RR_FASTFOOD_OLD") is not None  # read once per process by the library, so once here too
D2S = (1, 2, 4, 8, 16, 32, 64, 128, 256)
POW2_NORM = (1, 4, 16, 64, 256)  # d2^-1.5 is a power of two: S d2^-1.5 is exact, so is the comparison

# Largest |error| of the hardware v_sin_f32 / v_cos_f32 on all multiples of 2^-16 in [-1/2, 1/2] revolutions against float64,
# measured by tools/probes/sincos_probe.hip on an MI355X (docs/KERNELS.md 3.7): 1.171961e-07 = 1.97 x 2^-24 for the sine (at
# t = -0.25764) and the same for the cosine (at t = -0.00764), rounded up here.
SINCOS_F32_MAX_ERR = 1.172e-7
# float32 features at an exactly known phase: twice the probe's maximum, plus 2^-23 for the multiply by float32(1 / sqrt n)
# (2^-24 for the factor's own rounding, 2^-24 for the product's) on values of at most one
PHI_F32_BOUND = 2 * SINCOS_F32_MAX_ERR + 2.0 ** -23
# float64 features: below 3 ulp of unit amplitude -- the fdlibm kernels of rr_sincos_rev_f64 give under 1 ulp, the rounding of
# the 2 pi f argument at most 0.8 ulp (|2 pi f| <= pi / 4 after the quarter-turn reduction), the scale multiply 0.5
PHI_F64_BOUND = 1e-15


# ---- the instance table ---------------------------------------------------------------------------------------------------
def instance(compute, d2, d, k, ldx, ldo, x_align, out_align, mode, old=False):
    """(family, R, VEC, FULL) of the kernel ff_launch runs: compute "f32" / "f64", x_align / out_align the offsets IN ELEMENTS
    of the X and output pointers from a vector-aligned address (device allocations are 256-byte aligned), mode "vx" / "phi" /
    "gm".  VEC and FULL are the template arguments of the launched instance (None for the lane-minor kernel, which has no
    such variants): VEC = rows, row width and both pointers fit vw-element vector accesses; FULL = VEC and k % 4 == 0 (the
    scalar launch is always the partial-wave instance).  `old`: RR_FASTFOOD_OLD is set (ignored by the mixture mode)."""
    assert compute in ("f32", "f64") and mode in ("vx", "phi", "gm") and d2 in D2S and 1 <= d <= d2 and k >= 1
    if mode == "gm" and not 16 <= d2 <= 256:
        raise ValueError("RR_ERR_UNSUPPORTED")
    if 16 <= d2 <= 256 and (mode == "gm" or not old):
        R = d2 // 16
        vw = min(4 if compute == "f32" else 2, R)
        vec = ldx % vw == 0 and ldo % vw == 0 and d % vw == 0 and x_align % vw == 0 and out_align % vw == 0
        full = k % 4 == 0
        return ("rr_fastfood16_kernel" if compute == "f32" else "rr_fastfood16d_kernel", R, vec, vec and full)
    return ("rr_fastfood_kernel", 1 if d2 <= 64 else d2 // 64, None, None)


def ident(inst, mode):
    """The identifier the bounds-checking build counts a launch of this instance under."""
    fam, R, vec, full = inst
    s = "%s/R%d/%s" % (fam, R, mode)
    return s if vec is None else s + ("/vec" if vec else "/scalar") + ("/full" if full else "/partial")


def all_idents():
    out = []
    for mode in ("vx", "phi", "gm"):
        for R in (1, 2, 4, 8, 16):
            for fam in ("rr_fastfood16_kernel", "rr_fastfood16d_kernel"):
                out += [ident((fam, R, v, f), mode) for v, f in ((True, True), (True, False), (False, False))]
            out.append(ident(("rr_fastfood_kernel", R, None, None), mode))
    return out


# ---- the integer oracle ---------------------------------------------------------------------------------------------------
def hadamard_pm1(n):
    """Natural-order (Sylvester) Hadamard matrix, entries +-1, int64."""
    i = np.arange(n)
    bits = i[:, None] & i[None, :]
    par = np.zeros_like(bits)
    while bits.any():
        par ^= bits & 1
        bits = bits >> 1
    return (1 - 2 * par).astype(np.int64)


def int_chain(X, inv_ls, B, G, PI, blas=False):
    """(I, A): I = H((H(x / l o B_j))[PI_j] o G_j) per block in int64 (no normalisation, no S), shape (N, k d2), and the same
    chain over absolute values, which bounds every partial sum of every summation order.  blas: run the products in float64
    (exact below 2^53, asserted) for the one case too large for integer loops."""
    X = np.asarray(X)
    assert np.array_equal(X, np.rint(X))
    k, d2 = B.shape
    N, d = X.shape
    T = np.float64 if blas else np.int64
    H = hadamard_pm1(d2).astype(T)
    Xp = np.zeros((N, d2), dtype=T)
    Xp[:, :d] = (X.astype(np.int64) * np.asarray(inv_ls, dtype=np.int64)).astype(T)
    aH = np.abs(H)
    aX = np.abs(Xp) @ aH
    I = np.empty((N, k * d2), dtype=np.int64)
    A = np.empty((N, k * d2), dtype=np.int64)
    for j in range(k):
        v = (Xp * B[j].astype(T)) @ H
        I[:, j * d2:(j + 1) * d2] = ((v[:, PI[j]] * G[j].astype(T)) @ H).astype(np.int64)
        A[:, j * d2:(j + 1) * d2] = ((aX[:, PI[j]] * np.abs(G[j]).astype(T)) @ aH).astype(np.int64)
    assert not blas or A.max() < EXACT["f64"]
    return I, A


def int_data(seed, N, d, d2, k, ard=True):
    """x in [-3, 3] (every row its own pattern), 1 / l in {1, 2, 4}, B = +-1, G in [-3, 3], PI a permutation per block."""
    rs = np.random.RandomState(seed)
    X = rs.randint(-3, 4, size=(N, d))
    inv_ls = rs.choice([1, 2, 4], size=d) if ard else rs.choice([1, 2, 4], size=1)
    B = rs.randint(2, size=(k, d2)) * 2 - 1
    G = rs.randint(-3, 4, size=(k, d2))
    PI = np.array([rs.permutation(d2) for _ in range(k)])
    S_int = rs.randint(1, 5, size=(k, d2)).astype(np.float64)
    return X, inv_ls, B, G, PI, S_int


def dyadic_S(d2):
    """S with float32(S d2^-1.5 / 2 pi) == 2^-4 exactly -- checked with the library's own inv2pi and with d2^-1.5 one ulp either
    side of Python's (the library's pow() may round differently).  Returns (S, Srev64 as the library forms it)."""
    norm = float(d2) ** -1.5
    S = 2 * np.pi * 2.0 ** -4 / norm
    for nm in (np.nextafter(norm, 0), norm, np.nextafter(norm, 1)):
        assert np.float32((S * nm) * INV2PI) == np.float32(2.0 ** -4), d2
    return S, (S * norm) * INV2PI


def dyadic_mean(m):
    """mean = 2 pi 2^-4 m for small integers m, nudged by at most a few ulp so that the library's mean * inv2pi is EXACTLY
    m / 16 in float64 (hence in float32): mX and ph +- mX are then exact in both arithmetics."""
    m = np.asarray(m, dtype=np.float64)
    base = 2 * np.pi * 2.0 ** -4
    cands = [base]
    for _ in range(4):
        cands = [np.nextafter(cands[0], 0)] + cands + [np.nextafter(cands[-1], 1)]
    good = [c for c in cands if c * INV2PI == 2.0 ** -4]
    assert good, "no float64 near 2 pi / 16 maps to 1/16"
    mean = good[len(good) // 2] * m
    assert np.array_equal(mean * INV2PI, m / 16) and np.array_equal((mean * INV2PI).astype(np.float32), (m / 16).astype(np.float32))
    return mean


# ---- cases ----------------------------------------------------------------------------------------------------------------
# api "host": rr_fastfood_vx / _transform / _gm_transform (ldx = d, ldo = width, aligned buffers of the library's own);
# api "dev": rr_fastfood_transform_dev / _gm_transform_dev with ldx = d + ldx_extra, ldphi = width + ldo_extra and the X / output
# pointers x_off / out_off elements into their buffers
# sfrac (VX only): S = integer + 2^-30, so that S d2^-1.5 is NOT a float32 -- a float32 table or route shows in a float64 output
Case = namedtuple("Case", "label compute d2 d k N mode api xdt odt ldx_extra ldo_extra x_off out_off ard sfrac")


def _case(label, compute, d2, d, k, N, mode, api="host", xdt=None, odt=None, ldx_extra=0, ldo_extra=0, x_off=0, out_off=0, ard=True,
          sfrac=False):
    assert not sfrac or mode == "vx"
    return Case(label, compute, d2, d, k, N, mode, api, xdt or compute, odt or compute, ldx_extra, ldo_extra, x_off, out_off, ard,
                sfrac)


def width_of(c):
    return {"vx": 1, "phi": 2, "gm": 4}[c.mode] * c.d2 * c.k


def case_instance(c, old=False):
    w = width_of(c)
    return instance(c.compute, c.d2, c.d, c.k, c.d + c.ldx_extra, w + c.ldo_extra, c.x_off, c.out_off, c.mode, old=old)


def grid_cases():
    """Every d2, every launch variant per register count, every mode, both arithmetics -- host-buffer calls, 11 rows."""
    out = []
    for compute in ("f32", "f64"):
        for d2 in D2S:
            if d2 < 16:
                shapes = [(d2, 1), (max(1, d2 - 3), 5)]
            else:
                vw = min(4 if compute == "f32" else 2, d2 // 16)
                kp = {16: 5, 32: 6, 64: 7, 128: 2, 256: 1}[d2]
                shapes = [(d2 - 4, 4), (d2, kp), (d2 - 4, kp + 4 if kp < 4 else 3)]  # vec/full, vec/partial twice
                if vw > 1:
                    shapes += [(d2 - 3, 4), (d2 - 5, 3)]  # d % vw != 0: scalar accesses, whole and part waves
                if d2 == 256:
                    shapes += [(256, 2), (252, 3)]  # k < 4 at R = 16: one, two and three idle DPP rows
            for d, k in shapes:
                for mode in ("vx", "phi", "gm"):
                    if mode == "gm" and d2 < 16:
                        continue
                    out.append(_case("grid/%s/d2=%d/d=%d/k=%d/%s" % (compute, d2, d, k, mode), compute, d2, d, k, 11, mode,
                                     ard=(d + k) % 2 == 0))
    return out


def dtype_cases():
    """All eight x_dtype x compute x out_dtype combinations of ff_dispatch at one shape per family.  With integer S the float32
    and the float64 product I * (S d2^-1.5) are the same number wherever I S < 2^24 and d2^-1.5 is a power of two, so VX runs a
    second time with S = integer + 2^-30: S d2^-1.5 then needs more than 24 bits, and a float64 basis whose table or route is
    float32 misses the float64 output by 2^-32 relative -- bit for bit at d2 = 64, a million ulp at d2 = 8."""
    out = []
    for d2, d, k in ((8, 5, 3), (64, 40, 3)):
        for xdt in ("f32", "f64"):
            for compute in ("f32", "f64"):
                for odt in ("f32", "f64"):
                    for mode in ("vx", "phi") + (("gm",) if d2 >= 16 else ()):
                        out.append(_case("dtype/x=%s/c=%s/o=%s/d2=%d/%s" % (xdt, compute, odt, d2, mode), compute, d2, d, k, 13,
                                         mode, xdt=xdt, odt=odt))
                    out.append(_case("dtype/x=%s/c=%s/o=%s/d2=%d/vx+2^-30" % (xdt, compute, odt, d2), compute, d2, d, k, 13, "vx",
                                     xdt=xdt, odt=odt, sfrac=True))
    return out


ROW_COUNTS = (1, 2, 3, 4, 5, 6, 7, 9)


def row_cases():
    """Row-pipeline edges: one to nine rows (the clamp rp >= 4 runs N = 5 as blocks of 4 rows and 1 row), and a prime row count
    with k = 1, so that several row blocks arise and the last one is ragged at any occupancy."""
    out = []
    for compute in ("f32", "f64"):
        for N in ROW_COUNTS:
            for mode in ("vx", "phi", "gm"):
                out.append(_case("rows/%s/N=%d/%s" % (compute, N, mode), compute, 64, 40, 3, N, mode))
        out.append(_case("rows/%s/N=20011/vx" % compute, compute, 16, 12, 1, 20011, "vx"))
        out.append(_case("rows/%s/N=20011/phi" % compute, compute, 16, 12, 1, 20011, "phi"))
    return out


def variant_cases():
    """Device-resident calls whose leading dimensions or pointers flip VEC on their own; sentinel-filled output buffers."""
    out = []
    flips = [("aligned", {}), ("ldx+1", {"ldx_extra": 1}), ("ldo+1", {"ldo_extra": 1}), ("ldo+4", {"ldo_extra": 4}),
             ("x+1", {"x_off": 1}), ("out+1", {"out_off": 1})]
    for compute in ("f32", "f64"):
        for d2, d in ((64, 40), (32, 20), (16, 12)):
            for k in (4, 3):
                for mode in ("phi", "gm"):
                    for name, kw in flips:
                        if d2 != 64 and name in ("ldx+1", "x+1"):
                            continue
                        out.append(_case("dev/%s/d2=%d/k=%d/%s/%s" % (compute, d2, k, mode, name), compute, d2, d, k, 10, mode,
                                         api="dev", **kw))
    # the other dtypes of X and of the output through the device-resident route
    out.append(_case("dev/f32/x=f64/o=f64/out+1", "f32", 64, 40, 3, 10, "phi", api="dev", xdt="f64", odt="f64", out_off=1))
    out.append(_case("dev/f64/x=f32/o=f32/ldo+1", "f64", 64, 40, 3, 10, "gm", api="dev", xdt="f32", odt="f32", ldo_extra=1))
    return out


def old_cases():
    """RR_FASTFOOD_OLD=1: the lane-minor kernel at 16 <= d2 <= 256 -- the only way rr_fastfood_kernel<2> and <4> ever run."""
    out = []
    for compute in ("f32", "f64"):
        for d2, d, k in ((16, 12, 5), (64, 40, 3), (128, 101, 2), (256, 200, 3)):
            for mode in ("vx", "phi"):
                out.append(_case("old/%s/d2=%d/%s" % (compute, d2, mode), compute, d2, d, k, 11, mode))
    return out


GRID, DTYPES, ROWS, VARIANTS, OLD_CASES = grid_cases(), dtype_cases(), row_cases(), variant_cases(), old_cases()
ALL_CASES = GRID + DTYPES + ROWS + VARIANTS


def _ids(cases):
    return [c.label for c in cases]


# ---- running a case and checking it ------------------------------------------------------------------------------------------
SENTINEL = {4: np.uint32(0xC2F7A5A5), 8: np.uint64(0xC2F7A5A5C2F7A5A5)}
_HANDLES = {}


def _seed(c):
    return (c.d2 * 131 + c.d * 17 + c.k * 7 + c.N) % (1 << 31)


def case_data(c):
    """Integer data of a case, its S (integers for VX, the dyadic constant for features), mean (mixture mode) and reference."""
    X, inv_ls, B, G, PI, S_int = int_data(_seed(c), c.N, c.d, c.d2, c.k, c.ard)
    I, A = int_chain(X, inv_ls, B, G, PI, blas=c.N * c.k * c.d2 > (1 << 23))
    assert A.max() < EXACT[c.compute], (c.label, int(A.max()))
    S = (S_int + 2.0 ** -30 if c.sfrac else S_int) if c.mode == "vx" else np.full((c.k, c.d2), dyadic_S(c.d2)[0])
    m = M = mean = None
    if c.mode == "gm":
        m = np.random.RandomState(_seed(c) + 1).randint(-2, 3, size=c.d)
        mean = dyadic_mean(m)
        M = X.astype(np.int64) @ m
        assert (A.max() + np.abs(X).astype(np.int64) @ np.abs(m)).max() < EXACT[c.compute]
    return SimpleNamespace(X=X, ls=1.0 / inv_ls, B=B, G=G, PI=PI, S=S, I=I, A=A, m=m, M=M, mean=mean)


def _handle(c, D):
    from revrand_amd import _hip
    return _hip.FastFoodHandle(c.d, c.d2, c.k, D.B, D.G, D.PI, D.S, compute=c.compute)


def run_case(c, D):
    """The case's output (N, width) in its output dtype.  Device-resident calls check on the way that every byte of the
    sentinel-filled buffer outside the written block -- before an offset output, the columns beyond `width`, two rows beyond
    N -- still holds the sentinel."""
    from revrand_amd import _hip
    ff = _handle(c, D)
    X = D.X.astype(NP[c.xdt])
    odt = NP[c.odt]
    w = width_of(c)
    if c.api == "host":
        assert not (c.ldx_extra or c.ldo_extra or c.x_off or c.out_off)
        if c.mode == "vx":
            return ff.vx(X, D.ls, out_dtype=odt)
        if c.mode == "phi":
            return ff.transform(X, D.ls, out_dtype=odt)
        return ff.gm_transform(X, D.mean, D.ls, out_dtype=odt)
    dev = ff.dev
    ldx, ldo = c.d + c.ldx_extra, w + c.ldo_extra
    xs, osz = X.dtype.itemsize, np.dtype(odt).itemsize
    flat = np.full(c.x_off + c.N * ldx, 7.0, dtype=X.dtype)  # (pad elements of X hold a value that would show if read)
    flat[c.x_off:].reshape(c.N, ldx)[:, :c.d] = X
    bx = dev.upload_vector(flat)
    dX = SimpleNamespace(ptr=ctypes.c_void_p(bx.ptr.value + c.x_off * xs), dtype=X.dtype, shape=(c.N, c.d), ld=ldx)
    total = c.out_off + (c.N + 2) * ldo
    bo = dev.upload_vector(np.full(total, SENTINEL[osz]))
    po = ctypes.c_void_p(bo.ptr.value + c.out_off * osz)
    try:
        if c.mode == "phi":
            ff.transform_dev(dX, D.ls, po, out_dtype=odt, ldphi=ldo)
        else:
            ff.gm_transform_dev(dX, D.mean, D.ls, po, out_dtype=odt, ldphi=ldo)
        dev.sync()
        raw = dev.download(bo, (total,), SENTINEL[osz].dtype)
    finally:
        bx.free()
        bo.free()
    body = raw[c.out_off:].reshape(c.N + 2, ldo)
    assert np.all(raw[:c.out_off] == SENTINEL[osz]), "%s: bytes before the output were written" % c.label
    assert np.all(body[:c.N, w:] == SENTINEL[osz]), "%s: columns beyond the written width were written" % c.label
    assert np.all(body[c.N:] == SENTINEL[osz]), "%s: rows beyond N were written" % c.label
    return np.ascontiguousarray(body[:c.N, :w]).view(odt)


def check_vx(c, D, got):
    """VX = T(I) * T(S d2^-1.5), one multiply in the compute type, cast to the output type: bit for bit where d2^-1.5 is a power
    of two; elsewhere within one ulp of the coarser of the two types (the library's pow() may round d2^-1.5 the other way:
    one ulp of the compute type, which the monotone cast turns into at most one ulp of the output type)."""
    T, O = NP[c.compute], NP[c.odt]
    want_T = D.I.astype(T) * np.tile((D.S * float(c.d2) ** -1.5).astype(T).ravel(), (c.N, 1))
    want = want_T.astype(O)
    assert got.dtype == O and got.shape == want.shape
    if c.d2 in POW2_NORM:
        bad = got != want
        print("%-44s VX bit for bit: %d of %d differ" % (c.label, int(bad.sum()), bad.size))
        assert not bad.any(), "%s: %d of %d differ, max |diff| %g" % (c.label, int(bad.sum()), bad.size, np.abs(got - want).max())
    else:
        ulp = np.maximum(np.spacing(np.abs(want_T)).astype(np.float64), np.spacing(np.abs(want)).astype(np.float64))
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp
        print("%-44s VX max error %.2f ulp" % (c.label, err.max()))
        assert err.max() <= 1.0, (c.label, err.max())


def _exact_cos_sin(t, extra=0.0):
    """cos, sin of 2 pi (t + extra) for float64 revolutions t and a tiny float64 correction: the reduction t - rint(t) is exact,
    the rest in long double."""
    f = (t - np.rint(t)).astype(np.longdouble) + extra
    return np.cos(TWO_PI_L * f), np.sin(TWO_PI_L * f)


def phi_reference(c, D):
    """(blocks, |ph|, |mx|): the [cos | sin] blocks (x 2 for the mixture mode) at the case's known phases, in long double, and the
    magnitudes of the chain's phase and of the mean shift in revolutions.
    float32 arithmetic: phase = I / 16 (+- M / 16), exact.
    float64, no mean: Srev64 is ~1e-17 off 2^-4, so the phase is float64(I) * Srev64 -- the kernel's own single multiply.
    float64, mixture mode: the kernel forms I * Srev64 +- M / 16, as a multiply and an add or -- the compiler's choice -- as one
    fused multiply-add; the two differ by a rounding at the size of the phase wherever Srev64 is not exactly 2^-4 (no S makes it
    so for d2 = 2, 8, 32, 128).  The reference is therefore the exact value, (I +- M) / 16 reduced exactly plus I * (Srev64 -
    2^-4), and phi_bound grants the roundings."""
    if c.compute == "f32":
        ph = D.I.astype(np.float64) / 16
    else:
        ph = D.I.astype(np.float64) * dyadic_S(c.d2)[1]
    mx = None
    if c.mode == "gm":
        mx = (D.M.astype(np.float64) / 16)[:, None]
        if c.compute == "f32":
            blocks = _exact_cos_sin(ph + mx) + _exact_cos_sin(ph - mx)
        else:
            I = D.I.astype(np.float64)
            extra = I * (dyadic_S(c.d2)[1] - 2.0 ** -4)  # (the difference is exact; |extra| ~ 1e-14: its own rounding is nothing)
            blocks = _exact_cos_sin(I / 16 + mx, extra) + _exact_cos_sin(I / 16 - mx, extra)
    else:
        blocks = _exact_cos_sin(ph)
    return np.concatenate(blocks, axis=1), np.abs(ph), None if mx is None else np.abs(mx)


def phi_bound(c, phase, mx=None):
    """Absolute bound on Phi sqrt(n) (sqrt(2n) in the mixture mode) per element at a known phase."""
    if c.compute == "f32":
        return np.full(phase.shape, PHI_F32_BOUND)
    b = np.full(phase.shape, PHI_F64_BOUND)
    if c.d2 not in POW2_NORM:
        b = b + 2 * np.pi * 2.0 ** -52 * phase  # one ulp of pow() in Srev64, times the phase, in radians
    if mx is not None and dyadic_S(c.d2)[1] != 2.0 ** -4:
        # mixture mode with an inexact product: half an ulp of |ph| for the multiply and half an ulp of |ph +- mx| <= |ph| + |mx|
        # for the add (the fused form has the second only), in radians
        b = b + 2 * np.pi * 2.0 ** -53 * (2 * phase + mx)
    if c.odt == "f32":
        b = b + 2.0 ** -24  # the output rounding of a value of at most one
    return b


def check_phi(c, D, got):
    n = c.d2 * c.k
    nblk = 4 if c.mode == "gm" else 2
    want, phase, mx = phi_reference(c, D)
    assert got.dtype == NP[c.odt] and got.shape == want.shape == (c.N, nblk * n)
    amp = np.sqrt(np.longdouble((2 if c.mode == "gm" else 1) * n))
    err = np.abs(got.astype(np.longdouble) * amp - want).astype(np.float64)
    bound = np.tile(phi_bound(c, phase, mx), (1, nblk))
    print("%-44s Phi max |error| %.3e (bound %.3e), max phase %.0f rev" % (c.label, err.max(), bound.min(), phase.max()))
    assert np.all(err <= bound), "%s: %d of %d beyond the bound, max |error| %g" % (c.label, int((err > bound).sum()), err.size, err.max())


def run_and_check(c):
    D = case_data(c)
    got = run_case(c, D)
    (check_vx if c.mode == "vx" else check_phi)(c, D, got)
    return D, got


# ---- CPU tests: the references and the coverage of the case list --------------------------------------------------------------
def test_int_chain_agrees_with_the_oracle():
    """int_chain * S * d2^-1.5 equals oracle.fastfood_VX (float64 butterflies, halved at every stage) to rounding, the bound
    stays below 2^24 at the largest block, and the float64-BLAS route equals the int64 one."""
    for d2, d, k, N in ((1, 1, 3, 5), (2, 2, 3, 5), (8, 5, 3, 7), (16, 12, 5, 9), (64, 40, 3, 11), (128, 101, 2, 6), (256, 256, 3, 40)):
        X, inv_ls, B, G, PI, S = int_data(d2 + N, N, d, d2, k)
        I, A = int_chain(X, inv_ls, B, G, PI)
        assert np.all(np.abs(I) <= A) and A.max() < 5e5 < EXACT["f32"]
        I2, A2 = int_chain(X, inv_ls, B, G, PI, blas=True)
        assert np.array_equal(I, I2) and np.array_equal(A, A2)
        ref = orc.fastfood_VX(X * inv_ls.astype(np.float64), B, G.astype(np.float64), PI, S)
        mine = I * np.tile(S.ravel(), (N, 1)) * float(d2) ** -1.5
        assert np.abs(mine - ref).max() <= 4e-16 * np.abs(ref).max(), (d2, np.abs(mine - ref).max() / np.abs(ref).max())
    H = hadamard_pm1(8)
    assert np.array_equal(H @ H, 8 * np.eye(8, dtype=np.int64))
    assert np.array_equal(orc.hadamard(np.eye(8), False) * 8, H)


def test_dyadic_phases_are_exact_on_the_host():
    """The constants behind the exactly known phases, with the library's own inv2pi literal."""
    for d2 in D2S:
        S, srev = dyadic_S(d2)
        assert abs(srev - 2.0 ** -4) < 1e-16 and np.float32(srev) == np.float32(2.0 ** -4)
    mean = dyadic_mean(np.arange(-2, 3))
    assert np.abs(mean - 2 * np.pi / 16 * np.arange(-2, 3)).max() < 1e-15


def reachable_instances():
    """{((family, R, VEC, FULL), mode)} that some call can launch: for the two lane-major families every register count in each
    launch variant -- (vec, full), (vec, partial), (scalar, partial); the scalar one does not exist at R = 1, where vw = 1 and
    every address is aligned -- in every mode; the lane-minor kernel at R = 1 (d2 < 16 by default) and at R = 1, 2, 4 under
    RR_FASTFOOD_OLD, without the mixture mode."""
    want = set()
    for fam in ("rr_fastfood16_kernel", "rr_fastfood16d_kernel"):
        for R in (1, 2, 4, 8, 16):
            for var in ((True, True), (True, False)) + (((False, False),) if R > 1 else ()):
                for mode in ("vx", "phi", "gm"):
                    want.add(((fam, R) + var, mode))
    for R in (1, 2, 4):
        for mode in ("vx", "phi"):
            want.add((("rr_fastfood_kernel", R, None, None), mode))
    return want


def reachable_idents():
    return {ident(*key) for key in reachable_instances()}


def test_cases_reach_every_reachable_instance():
    """The case list, routed by `instance`: every d2, both arithmetics, every mode; for the two lane-major families every
    register count in each launch variant -- (vec, full), (vec, partial), (scalar, partial); the scalar one does not exist at
    R = 1, where vw = 1 and every address is aligned -- and each variant in every mode; the lane-minor kernel at R = 1 by
    default and at R = 1, 2, 4 under RR_FASTFOOD_OLD; k = 1, 2, 3 at R = 16; each alignment rule flips VEC on its own."""
    hit = {}
    for c in ALL_CASES:
        hit.setdefault((case_instance(c), c.mode), c.label)
    for c in OLD_CASES:
        hit.setdefault((case_instance(c, old=True), c.mode), c.label)
    want = reachable_instances()
    for key in sorted(want, key=str):
        print("%-48s %s" % (ident(*key), hit.get(key, "NOT HIT")))
    assert want <= set(hit), sorted(ident(*k) for k in want - set(hit))
    assert set(ident(*k) for k in hit) <= set(all_idents())
    for compute in ("f32", "f64"):
        assert {c.d2 for c in ALL_CASES if c.compute == compute} == set(D2S)
        assert {c.k for c in ALL_CASES if c.compute == compute and c.d2 == 256 and c.k < 4} == {1, 2, 3}
        assert {(c.xdt, c.odt) for c in DTYPES if c.compute == compute} == {(a, b) for a in ("f32", "f64") for b in ("f32", "f64")}
    # each of the five conditions behind VEC decides on its own
    base = dict(compute="f32", d2=64, d=40, k=4, ldx=40, ldo=512, x_align=0, out_align=0, mode="phi")
    assert instance(**base)[2:] == (True, True)
    for kw in ({"ldx": 41}, {"ldo": 513}, {"d": 39}, {"x_align": 1}, {"out_align": 1}):
        assert instance(**dict(base, **kw))[2:] == (False, False), kw
    assert instance(**dict(base, ldo=516))[2:] == (True, True) and instance(**dict(base, k=3))[2:] == (True, False)
    assert instance(**dict(base, compute="f64", x_align=2))[2] and not instance(**dict(base, compute="f64", out_align=1))[2]
    flips = {c.label.rsplit("/", 1)[1]: case_instance(c)[2] for c in VARIANTS if c.label.startswith("dev/f32/d2=64/k=4/phi/")}
    assert flips == {"aligned": True, "ldx+1": False, "ldo+1": False, "ldo+4": True, "x+1": False, "out+1": False}, flips
    with pytest.raises(ValueError):
        instance("f32", 8, 5, 3, 5, 96, 0, 0, "gm")


# ---- GPU tests --------------------------------------------------------------------------------------------------------------
gpu = pytest.mark.gpu


@gpu
@pytest.mark.parametrize("c", GRID, ids=_ids(GRID))
def test_every_instance_is_exact(c):
    """VX bit for bit (one ulp where d2^-1.5 is not a power of two) and Phi at exactly known phases, for every d2, launch variant
    and mode in both arithmetics."""
    run_and_check(c)


@gpu
@pytest.mark.parametrize("c", DTYPES, ids=_ids(DTYPES))
def test_every_dtype_combination_is_exact(c):
    """The eight x_dtype x compute x out_dtype cases of ff_dispatch at one shape per family.  What tells a float64 basis on the
    float32 route (or with a float32 table) apart: the VX cases with S = integer + 2^-30 and a float64 output (with integer S
    the two products are the same number at these shapes), and the float64-output feature cases, whose 1e-15 no float32 sine
    meets."""
    run_and_check(c)


@gpu
@pytest.mark.parametrize("c", ROWS, ids=_ids(ROWS))
def test_row_pipeline_edges(c):
    """One to nine rows and a prime row count: every row is its own integer pattern, so a misplaced, skipped or doubled row of
    the two-rows-ahead pipeline shows."""
    D, _ = run_and_check(c)
    assert c.N == 1 or len({r.tobytes() for r in D.I}) > min(c.N, 1000) // 2  # (the rows really differ)


RP_CASES = {rp: [_case("rp=%d/%s" % (rp, mode), "f32", 64, 40, 3, 23, mode) for mode in ("vx", "phi", "gm")] for rp in (1, 2, 3, 5)}
CLAMP_CASES = [_case("clamp/%s" % mode, "f32", 16, 12, 1, 70001, mode) for mode in ("vx", "phi")]
SEAM_CASE = _case("seam", "f32", 128, 128, 64, 4100, "phi", xdt="f32", odt="f32")


@gpu
@pytest.mark.parametrize("rp", sorted(RP_CASES))
def test_rows_per_block_override(rp, monkeypatch):
    """RR_FF_ROWS_PER_BLOCK (read at every call by the float32 lane-major launcher, and by that one only: the float64 launcher
    has no such switch, so there is no float64 case): row blocks of 1, 2, 3 and 5 rows, odd ones storing their last row twice,
    23 rows so that the last block is ragged."""
    monkeypatch.setenv("RR_FF_ROWS_PER_BLOCK", str(rp))
    for c in RP_CASES[rp]:
        run_and_check(c)


@gpu
def test_grid_y_clamp(monkeypatch):
    """RR_FF_ROWS_PER_BLOCK=1 with 70 001 rows: more row blocks than the grid's y extent allows, so the launcher's clamp
    (> 65535) raises the rows per block to 2."""
    monkeypatch.setenv("RR_FF_ROWS_PER_BLOCK", "1")
    for c in CLAMP_CASES:
        run_and_check(c)


@gpu
def test_host_call_across_a_chunk_seam():
    """ff_host_call streams rows in chunks of 256 MiB / (bytes per row): d2 = 128, k = 64, float32 out is 66 048 bytes per
    row, 4064 rows per chunk, so 4100 rows cross one seam."""
    c = SEAM_CASE
    assert (256 << 20) // (c.d * 4 + width_of(c) * 4) < c.N
    run_and_check(c)


@gpu
@pytest.mark.parametrize("c", VARIANTS, ids=_ids(VARIANTS))
def test_variants_and_untouched_bytes(c):
    """Leading dimensions and pointer offsets that flip VEC on their own (the expected variant is asserted by the CPU test
    above and counted by the bounds build), through the device-resident calls into sentinel-filled buffers: the block is
    exact, every byte around it untouched."""
    run_and_check(c)


FEATMAT = [(compute, mode, col0) for compute in ("f32", "f64") for mode in ("phi", "gm") for col0 in (0, 4, 7, 256 + 3)]


def run_featmat(compute, mode, col0):
    """One feature-matrix case, checked; returns the instance the table names for the stored matrix's leading dimension."""
    from revrand_amd import _hip
    c = _case("featmat/%s/col0=%d/%s" % (compute, col0, mode), compute, 64, 40, 3, 37, mode, xdt="f32", odt="f32")
    D = case_data(c)
    ff = _handle(c, D)
    dev = ff.dev
    w = width_of(c)
    F = col0 + w + 5
    fm = _hip.FeatureMatrix(c.N, F)
    dX = dev.upload_matrix(D.X.astype(np.float32))
    fm.begin(c.N)
    if col0:
        dL = dev.upload_matrix(np.random.RandomState(col0).randn(c.N, col0).astype(np.float32))
        fm.put_linear(dL, False, 0)
    before = fm.download().view(np.uint32).copy()
    if mode == "phi":
        fm.put_fastfood(ff, dX, D.ls, col0)
    else:
        fm.put_fastfood_gm(ff, dX, D.mean, D.ls, col0)
    after = fm.download()
    inst = instance(compute, 64, 40, 3, 40, after.shape[1], 0, col0, mode)
    check_phi(c, D, np.ascontiguousarray(after[:, col0:col0 + w]))
    keep = np.ones(after.shape[1], dtype=bool)
    keep[col0:col0 + w] = False
    assert np.array_equal(after.view(np.uint32)[:, keep], before[:, keep])
    assert np.all(after[:, F:] == 0)
    return inst


@gpu
@pytest.mark.parametrize("compute,mode,col0", FEATMAT, ids=["%s-%s-col0=%d" % f for f in FEATMAT])
def test_feature_matrix_block_and_untouched_columns(compute, mode, col0):
    """rr_featmat_put_fastfood / _gm at column offsets that keep (0, 4) or break (7, 259) the vector alignment of the output,
    behind a linear child written first: the block at the exactly known phases, every other column of the stored matrix --
    the child, the columns not yet written, the pad columns -- bit-identical to its state before the call.  Which instance ran
    (the scalar one at 7 and 259) is what the bounds build's census counts."""
    run_featmat(compute, mode, col0)


# real-valued data: (N, d, nbases) -> d2 = 8 (lane-minor), 16, 32, 128, 256
REAL_SHAPES = [(50, 5, 24), (9, 16, 16 * 9), (33, 20, 32 * 5), (65, 100, 128 * 7), (17, 200, 256 * 3), (40, 128, 128 * 4)]


def _chain_ld(X, L, B, G, PI, Sv):
    """(value, absolute-value chain) of H((H(x L o B))[PI] o G) o Sv per block in long double (u = 2^-64), unnormalised H."""
    k, d2 = B.shape
    N, d = X.shape
    H = hadamard_pm1(d2).astype(np.longdouble)
    Xp = np.zeros((N, d2), dtype=np.longdouble)
    Xp[:, :d] = X.astype(np.longdouble) * L.astype(np.longdouble)
    aX = np.abs(Xp) @ np.abs(H)
    V = np.empty((N, k * d2), dtype=np.longdouble)
    A = np.empty((N, k * d2), dtype=np.longdouble)
    for j in range(k):
        v = (Xp * B[j]) @ H
        V[:, j * d2:(j + 1) * d2] = ((v[:, PI[j]] * G[j].astype(np.longdouble)) @ H) * Sv[j].astype(np.longdouble)
        A[:, j * d2:(j + 1) * d2] = ((aX[:, PI[j]] * np.abs(G[j]).astype(np.longdouble)) @ np.abs(H)) * np.abs(Sv[j]).astype(np.longdouble)
    return V, A


@gpu
@pytest.mark.parametrize("compute", ["f32", "f64"])
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_real_valued_data_element_by_element(shape, compute):
    """Gaussian x, the matrices of oracle.fastfood_matrices, ARD length scales.  The reference is the chain in long double over
    the tables as the library forms them (1 / l, G and S d2^-1.5 rounded to the compute type: a wrong conversion shows as a
    mismatch), so what separates the kernel from it are the roundings of its own arithmetic: x L, log2(d2) butterflies, the
    product with G, log2(d2) butterflies, the product with S -- 2 log2(d2) + 3 of them, one more granted for the library's pow().
    Every element of VX is held to ((1 + u)^(2 log2 d2 + 4) - 1) A, A the same chain over absolute values: a forward bound for
    any summation order, nothing measured.  Phi is held to 2 pi times that bound on the phase in revolutions plus the
    sine / cosine bound at an exact phase."""
    from revrand_amd import _hip
    N, d, nb = shape
    T = NP[compute]
    u = U[compute]
    rs = np.random.RandomState(N + d)
    X = rs.randn(N, d).astype(T)
    ls = np.linspace(0.6, 1.7, d)
    B, G, PI, S = orc.fastfood_matrices(nb, d, 5)
    k, d2 = B.shape
    ff = _hip.FastFoodHandle(d, d2, k, B, G, PI, S, compute=compute)
    L = (1.0 / ls).astype(T)
    norm = float(d2) ** -1.5
    # (1 + u)^m - 1 without forming 1 + u (which is 1 in float64 for u = 2^-53), + the long double reference's own error
    gamma = float(np.expm1((2 * int(np.log2(d2)) + 4) * np.log1p(u))) + 2.0 ** -60
    V, A = _chain_ld(X, L, B, G.astype(T), PI, (S * norm).astype(T))
    got = ff.vx(X, ls, out_dtype=T)
    err = np.abs(got.astype(np.longdouble) - V)
    ratio = float((err / (gamma * A + np.finfo(np.longdouble).tiny)).max())
    print("VX  %s %s: max error / bound %.3f" % (shape, compute, ratio))
    assert np.all(err <= gamma * A), ratio
    # features: phases in revolutions from the Srev table
    Vr, Ar = _chain_ld(X, L, B, G.astype(T), PI, ((S * norm) * INV2PI).astype(T))
    f = Vr - np.rint(Vr)
    want = np.concatenate((np.cos(TWO_PI_L * f), np.sin(TWO_PI_L * f)), axis=1)
    got = ff.transform(X, ls, out_dtype=T)
    err = np.abs(got.astype(np.longdouble) * np.sqrt(np.longdouble(d2 * k)) - want)
    trig = PHI_F32_BOUND if compute == "f32" else PHI_F64_BOUND
    bound = np.tile(2 * np.pi * gamma * Ar + trig, (1, 2))
    ratio = float((err / bound).max())
    print("Phi %s %s: max error / bound %.3f, max |error| %.3e" % (shape, compute, ratio, float(err.max())))
    assert np.all(err <= bound), ratio


@gpu
@pytest.mark.parametrize("compute", ["f32", "f64"])
def test_zero_mean_gives_two_identical_halves(compute):
    c = _case("gm0/%s" % compute, compute, 128, 100, 5, 21, "gm")
    D = case_data(c)
    D.mean, D.M = np.zeros(c.d), np.zeros(c.N, dtype=np.int64)
    got = run_case(c, D)
    n = c.d2 * c.k
    assert np.array_equal(got[:, :2 * n], got[:, 2 * n:])
    check_phi(c, D, got)


def run_old():
    """Entry point of the RR_FASTFOOD_OLD=1 subprocess: the exact VX and the exactly-known-phase cases at d2 = 16 .. 256."""
    assert OLD
    for c in OLD_CASES:
        assert case_instance(c, old=True)[0] == "rr_fastfood_kernel"
        run_and_check(c)
    print("OLD OK %d" % len(OLD_CASES))


@gpu
def test_old_lane_minor_kernel_is_exact():
    """RR_FASTFOOD_OLD=1 is read once per process: one subprocess runs the lane-minor kernel at d2 = 16, 64, 128, 256 -- the
    only way its R = 2 and R = 4 instances ever run -- through the same exact checks."""
    code = ("import sys; sys.path[:0] = [%r, %r, %r]\nimport test_gpu_fastfood_exact as M\nM.run_old()\n"
            % (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, RR_FASTFOOD_OLD="1"), capture_output=True,
                       text=True, timeout=900)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "OLD OK %d" % len(OLD_CASES) in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


# ---- which instance ran (the bounds-checking build's launch counts; tests/test_debug_builds.py) -------------------------------
def census_runs():
    """[(label, environment, run)]: every case that launches a chain kernel -- the case lists, the rows-per-block, grid-y clamp
    and chunk-seam cases and the feature-matrix cases (under RR_FASTFOOD_OLD the OLD cases); run() returns the identifier the
    table names."""
    def of(c):
        def run():
            run_case(c, case_data(c))
            return ident(case_instance(c, old=OLD), c.mode)
        return run
    if OLD:
        return [(c.label, {}, of(c)) for c in OLD_CASES]
    runs = [(c.label, {}, of(c)) for c in ALL_CASES]
    runs += [(c.label, {"RR_FF_ROWS_PER_BLOCK": str(rp)}, of(c)) for rp in sorted(RP_CASES) for c in RP_CASES[rp]]
    runs += [(c.label, {"RR_FF_ROWS_PER_BLOCK": "1"}, of(c)) for c in CLAMP_CASES]
    runs.append((SEAM_CASE.label, {}, of(SEAM_CASE)))
    for f in FEATMAT:
        runs.append(("featmat/%s/%s/col0=%d" % f, {}, lambda f=f: ident(run_featmat(*f), f[1])))
    return runs


def census():
    """Launches per FastFood instance for every entry of census_runs, under a library that counts them
    (rr_debug_kernel_launches): [(label, {identifier: launches, nonzero only}, identifier the table names)]."""
    from revrand_amd import _hip
    dev = _hip.get_device()
    lib = dev.lib
    assert lib.rr_debug_kernel_launches(None) == 0
    names = all_idents()
    out = []
    for label, env, run in census_runs():
        os.environ.update(env)
        try:
            dev.sync()
            lib.rr_debug_kernel_launches(None)
            want = run()
            dev.sync()
        finally:
            for key in env:
                del os.environ[key]
        got = {n: int(lib.rr_debug_kernel_launches(n.encode())) for n in names}
        out.append((label, {n: v for n, v in got.items() if v}, want))
    return out
