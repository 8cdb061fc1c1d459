"""Cases, data and checks for the mixture mode of the wide FastFood chain kernel (rr_fastfood64_kernel<..., GM>: d2 = 512, 1024,
2048, 4096 on handles of rr_fastfood_create_wide_gm), shared by tests/test_fastfood_gm_wide_host.py (CPU),
tests/test_gpu_fastfood_gm_wide.py and tests/test_gpu_fastfood_gm_wide_debug.py.

No data generator of its own: a case runs on `fastfood_wide_cases.case_data` of the same shape in "phi" mode -- integer x with at
most 64 non-zeros per row, 1 / l in {1, 2, 4}, the dyadic S, so the chain's phase is I / 16 revolutions exactly -- plus
``mean = dyadic_mean(m)`` with m in {-2 .. 2} per dimension (RandomState(d2 + d)): mean / 2 pi is m / 16 exactly, M = X @ m is an
exact integer with |M| <= 64 * 3 * 2 = 384, and ph +- mX = (I +- M) / 16 is exact in both arithmetics.  1 / l != 1, so an mX
wrongly taken on x / l shows.  The reference, the bound and the feature-matrix and census drivers are those of
tests/test_gpu_fastfood_exact.py (`phi_reference`) and tests/fastfood_wide_cases.py, restated for four blocks."""
import ctypes
from types import SimpleNamespace

import numpy as np

import fastfood_wide_cases as wc
import test_gpu_fastfood_exact as ex
from test_gpu_fastfood_exact import EXACT, NP, PHI_F32_BOUND, PHI_F64_BOUND, SENTINEL, _case, width_of

FAMILY = wc.FAMILY
MODE = "gm"
M_MAX = 384


# ---- the instance table ---------------------------------------------------------------------------------------------------
def instance(compute, d2, d, k, ldx, ldo, x_align, out_align, mode=MODE):
    """(family, R, VEC, None) of the kernel ff_launch runs for the mixture mode on a wide-GM handle: the wide family's rule
    (R = d2 / 64; VEC = rows, row widths and both pointers fit vectors of 16 bytes of the compute type), no partial waves."""
    assert compute in ("f32", "f64") and d2 in wc.D2S and 1 <= d <= d2 and k >= 1 and mode == MODE
    vw = 4 if compute == "f32" else 2
    vec = ldx % vw == 0 and ldo % vw == 0 and d % vw == 0 and x_align % vw == 0 and out_align % vw == 0
    return (FAMILY, d2 // 64, vec, None)


def ident(inst):
    """The identifier the bounds-checking build counts a launch of this instance under."""
    fam, R, vec, full = inst
    assert full is None
    return "%s/R%d/gm/%s" % (fam, R, "vec" if vec else "scalar")


def all_idents():
    return [ident((FAMILY, R, v, None)) for R in (8, 16, 32, 64) for v in (True, False)]


def reachable_instances():
    """Every register count in both launch variants (per arithmetic: the identifier does not name it)."""
    return {(compute, (FAMILY, R, v, None)) for compute in ("f32", "f64") for R in (8, 16, 32, 64) for v in (True, False)}


def case_instance(c):
    w = width_of(c)
    return instance(c.compute, c.d2, c.d, c.k, c.d + c.ldx_extra, w + c.ldo_extra, c.x_off, c.out_off, c.mode)


# ---- data -------------------------------------------------------------------------------------------------------------------
def case_data(c):
    """`wc.case_data` of the same shape as a "phi" case, plus m, mean and M = X @ m; asserts |M| <= 384 and that |I| + |M| (in
    fact the absolute-value chain plus |X| @ |m|) stays below the exactness limit of the arithmetic."""
    assert c.mode == MODE
    D = wc.case_data(c._replace(mode="phi"))
    m = np.random.RandomState(c.d2 + c.d).randint(-2, 3, size=c.d)
    M = D.X.astype(np.int64) @ m
    aM = np.abs(D.X).astype(np.int64) @ np.abs(m)
    assert aM.max() <= M_MAX and np.abs(M).max() > 0
    assert (D.A.max(axis=1) + aM).max() < EXACT[c.compute], c.label
    return SimpleNamespace(X=D.X, ls=D.ls, B=D.B, G=D.G, PI=D.PI, S=D.S, I=D.I, A=D.A, m=m, M=M, mean=ex.dyadic_mean(m))


# ---- cases ------------------------------------------------------------------------------------------------------------------
def grid_cases():
    """Both arithmetics x every d2 through the host-buffer call: d = d2 (vector accesses), d2 - 1 and d2 / 2 + 1 (odd: the scalar
    variant, the second with whole groups beyond d), d2 / 2 + 4 (vector accesses with lanes and groups beyond d; dropped at
    4096 as in wc.grid_cases); N = 1, 2 (fewer rows than waves), 7, 37 (a ragged last round)."""
    out = []
    for compute in ("f32", "f64"):
        for d2 in wc.D2S:
            for d, k, N in ((d2, 4, 7), (d2 - 1, 3, 2), (d2 // 2 + 1, 1, 1), (d2, 5, 37), (d2 // 2 + 4, 3, 7)):
                if d2 == 4096 and d == d2 // 2 + 4:
                    continue
                out.append(_case("widegm/%s/d2=%d/d=%d/k=%d/N=%d" % (compute, d2, d, k, N), compute, d2, d, k, N, MODE))
    return out


FLIPS = [("aligned", {}), ("ldx+1", {"ldx_extra": 1}), ("ldo+1", {"ldo_extra": 1}), ("ldo+4", {"ldo_extra": 4}),
         ("x+1", {"x_off": 1}), ("out+1", {"out_off": 1})]


def variant_cases():
    """Device-resident calls whose leading dimensions or pointers flip VEC on their own; sentinel-filled output buffers."""
    return [_case("widegm/dev/%s/d2=%d/%s" % (compute, d2, name), compute, d2, d2, 3, 7, MODE, api="dev", **kw)
            for compute in ("f32", "f64") for d2 in wc.D2S for name, kw in FLIPS]


def dtype_cases():
    """All eight x_dtype x compute x out_dtype combinations of ff_dispatch at d2 = 512."""
    return [_case("widegm/dtype/x=%s/c=%s/o=%s" % (xdt, compute, odt), compute, 512, 512, 3, 7, MODE, xdt=xdt, odt=odt)
            for xdt in ("f32", "f64") for compute in ("f32", "f64") for odt in ("f32", "f64")]


GRID, VARIANTS, DTYPES = grid_cases(), variant_cases(), dtype_cases()
ALL_CASES = GRID + VARIANTS + DTYPES
# rows per workgroup forced to 9 (RR_FF_ROWS_PER_BLOCK) with ten rows, as wc.RP_CASES: every wave takes several rows, so the x
# fetched a row ahead and the mX formed from it must stay paired
RP = wc.RP
RP_CASES = [_case("widegm/rp=9/%s/d2=%d" % (compute, d2), compute, d2, d2, 3, RP + 1, MODE) for compute in ("f32", "f64")
            for d2 in wc.D2S]
ZERO_MEAN_CASES = [_case("widegm/zero-mean/%s/d2=%d" % (compute, d2), compute, d2, d2 - 1, 3, 7, MODE) for compute in ("f32", "f64")
                   for d2 in (512, 4096)]
HUGE_LS_CASE = _case("widegm/lenscale=1e60", "f32", 512, 512, 3, 7, MODE)


def ids(cases):
    return [c.label for c in cases]


# ---- running a case and checking it -----------------------------------------------------------------------------------------
def handle(c, D):
    from revrand_amd import _hip
    return _hip.FastFoodHandle(c.d, c.d2, c.k, D.B, D.G, D.PI, D.S, compute=c.compute, wide="gm")


def run_case(c, D, mean=None, ls=None):
    """The case's output (N, 4n) in its output dtype (`mean`, `ls`: instead of the data's).  Device-resident calls check on the
    way that every element of the sentinel-filled buffer outside the written block -- before an offset output, the columns
    beyond 4n, two rows beyond N -- still holds the sentinel."""
    ff = handle(c, D)
    mean = D.mean if mean is None else mean
    ls = D.ls if ls is None else ls
    X = D.X.astype(NP[c.xdt])
    odt = NP[c.odt]
    w = width_of(c)
    assert w == 4 * c.d2 * c.k and ff.gm_chain_ok and ff.wide_gm
    if c.api == "host":
        assert not (c.ldx_extra or c.ldo_extra or c.x_off or c.out_off)
        return ff.gm_transform(X, mean, ls, out_dtype=odt)
    dev = ff.dev
    ldx, ldo = c.d + c.ldx_extra, w + c.ldo_extra
    xs, osz = X.dtype.itemsize, np.dtype(odt).itemsize
    flat = np.full(c.x_off + c.N * ldx, 7.0, dtype=X.dtype)  # (pad elements of X hold a value that would show if read)
    flat[c.x_off:].reshape(c.N, ldx)[:, :c.d] = X
    bx = dev.upload_vector(flat)
    dX = SimpleNamespace(ptr=ctypes.c_void_p(bx.ptr.value + c.x_off * xs), dtype=X.dtype, shape=(c.N, c.d), ld=ldx)
    total = c.out_off + (c.N + 2) * ldo
    bo = dev.upload_vector(np.full(total, SENTINEL[osz]))
    try:
        ff.gm_transform_dev(dX, mean, ls, ctypes.c_void_p(bo.ptr.value + c.out_off * osz), out_dtype=odt, ldphi=ldo)
        dev.sync()
        raw = dev.download(bo, (total,), SENTINEL[osz].dtype)
    finally:
        bx.free()
        bo.free()
    body = raw[c.out_off:].reshape(c.N + 2, ldo)
    assert np.all(raw[:c.out_off] == SENTINEL[osz]), "%s: elements before the output were written" % c.label
    assert np.all(body[:c.N, w:] == SENTINEL[osz]), "%s: columns beyond the written width were written" % c.label
    assert np.all(body[c.N:] == SENTINEL[osz]), "%s: rows beyond N were written" % c.label
    return np.ascontiguousarray(body[:c.N, :w]).view(odt)


def phi_bound(c, phase, mx):
    """Absolute bound on Phi sqrt(2n) per element at the exactly known phases: what ex.phi_bound grants the narrow mixture mode,
    with the pow() term where d2^-1.5 is no power of two AT THE WIDE SIZES (wc.POW2_NORM, as wc.check_phi has it).
    float32: ph +- mX = (I +- M) / 16 is exact, so PHI_F32_BOUND alone.  float64: PHI_F64_BOUND; one ulp of pow() in Srev64 times
    the phase; Srev64 is ~1e-17 off 2^-4, so the product I * Srev64 rounds (half an ulp of |ph|) and so does the sum (half an
    ulp of |ph| + |mX|; the fused form has the second only); the rounding of a float32 output."""
    if c.compute == "f32":
        return np.full(phase.shape, PHI_F32_BOUND)
    b = np.full(phase.shape, PHI_F64_BOUND)
    if c.d2 not in wc.POW2_NORM:
        b = b + 2 * np.pi * 2.0 ** -52 * phase
    if ex.dyadic_S(c.d2)[1] != 2.0 ** -4:
        b = b + 2 * np.pi * 2.0 ** -53 * (2 * phase + mx)
    if c.odt == "f32":
        b = b + 2.0 ** -24
    return b


def check_phi(c, D, got):
    """The four blocks [cos+ | sin+ | cos- | sin-] scaled by sqrt(2n) against exact cos / sin at (I +- M) / 16 revolutions
    (float32 arithmetic) or I Srev64 +- M / 16 (float64), ex.phi_reference, element by element."""
    n = c.d2 * c.k
    want, phase, mx = ex.phi_reference(c, D)
    assert got.dtype == NP[c.odt] and got.shape == want.shape == (c.N, 4 * n)
    err = np.abs(got.astype(np.longdouble) * np.sqrt(np.longdouble(2 * n)) - want).astype(np.float64)
    bound = np.tile(phi_bound(c, phase, mx), (1, 4))
    print("%-44s Phi max |error| %.3e (bound %.3e), max phase %.0f rev, max |mX| %.1f rev" % (
        c.label, err.max(), bound.min(), phase.max(), mx.max()))
    assert np.all(err <= bound), "%s: %d of %d beyond the bound, max |error| %g" % (c.label, int((err > bound).sum()), err.size, err.max())


def run_and_check(c):
    D = case_data(c)
    got = run_case(c, D)
    check_phi(c, D, got)
    return D, got


# ---- the feature matrix --------------------------------------------------------------------------------------------------
FEATMAT = [("f32", 512, 7), ("f64", 1024, 8)]  # (arithmetic of the basis, d2, col0): a misaligned and an aligned block


def run_featmat(compute, d2, col0):
    """rr_featmat_put_fastfood_gm at a non-zero col0 behind a linear child: the block at the exactly known phases, every other
    column of the stored matrix bit-identical to its state before the call, pad columns zero; returns the instance."""
    from revrand_amd import _hip
    c = _case("widegm/featmat/%s/d2=%d/col0=%d" % (compute, d2, col0), compute, d2, d2, 3, wc.NMAX, MODE, xdt="f32", odt="f32")
    D = case_data(c)
    ff = handle(c, D)
    dev = ff.dev
    w = width_of(c)
    F = col0 + w + 5
    fm = _hip.FeatureMatrix(c.N, F)
    dX = dev.upload_matrix(D.X.astype(np.float32))
    fm.begin(c.N)
    dL = dev.upload_matrix(np.random.RandomState(col0).randn(c.N, col0).astype(np.float32))
    fm.put_linear(dL, False, 0)
    before = fm.download().view(np.uint32).copy()
    fm.put_fastfood_gm(ff, dX, D.mean, D.ls, col0)
    after = fm.download()
    inst = instance(compute, d2, d2, 3, d2, after.shape[1], 0, col0)
    check_phi(c, D, np.ascontiguousarray(after[:, col0:col0 + w]))
    keep = np.ones(after.shape[1], dtype=bool)
    keep[col0:col0 + w] = False
    assert np.array_equal(after.view(np.uint32)[:, keep], before[:, keep])
    assert np.all(after[:, F:] == 0)
    return inst


# ---- which instance ran (the bounds-checking build's launch counts) -------------------------------------------------------
def census_runs():
    """[(label, environment, run)]: every case that launches the mixture mode; run() returns the identifier the table names."""
    def of(c):
        def run():
            run_case(c, case_data(c))
            return ident(case_instance(c))
        return run
    runs = [(c.label, {}, of(c)) for c in ALL_CASES]
    runs += [(c.label, {"RR_FF_ROWS_PER_BLOCK": str(RP)}, of(c)) for c in RP_CASES]
    for f in FEATMAT:
        runs.append(("widegm/featmat/%s/d2=%d/col0=%d" % f, {}, lambda f=f: ident(run_featmat(*f))))
    return runs


def census():
    """Launches per instance of the wide family (all three modes) and of the narrow families, which must not run at all, for
    every entry of census_runs, under a library that counts them (rr_debug_kernel_launches): [(label, {identifier: launches},
    identifier the table names)]."""
    import os
    from revrand_amd import _hip
    dev = _hip.get_device()
    lib = dev.lib
    assert lib.rr_debug_kernel_launches(None) == 0
    names = all_idents() + wc.all_idents() + ex.all_idents()
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
