"""Cases, data and checks for the wide FastFood chain kernel (rr_fastfood64_kernel: d2 = 512, 1024, 2048, 4096), shared by
tests/test_fastfood_wide_host.py (CPU) and tests/test_gpu_fastfood_wide.py.  The integer oracle, the dyadic phases and the
feature bounds are those of tests/test_gpu_fastfood_exact.py, imported from there.

What differs from the narrow blocks:

* Dense x in [-3, 3] no longer keeps the chain below 2^24 (12 * 4096 * 3 * 4096 ~ 6e8), so a row of x has AT MOST 64
  non-zeros: sum |x / l| <= 64 * 3 * 4 = 768 and every intermediate is at most 768 * 3 * 4096 ~ 9.4e6 < 2^24.  Each case still
  asserts its own bound from `int_chain`'s absolute-value chain.
* The non-zero positions of EVERY row hold column 0, column d - 1 and both sides of every 256-element boundary below d (the
  seams between a lane's register groups in float32: 64 lanes x 4 elements; every second one of float64's 128-element seams);
  the other positions are pairs (b - 1, b) around lane boundaries b (multiples of 2: every float64 lane boundary, every
  second one a float32 lane boundary), sixteen pairs per row dealt round-robin over the rows from a shuffled list of all of
  them.  With 2047 lane boundaries at d = 4096 and 64 non-zeros per row no ROW can carry every boundary; the data of the
  shapes d = d2 has as many rows as it takes to deal the whole list once (37 at d2 = 512, 1024; 64 at 2048; 127 at 4096), and
  COVER_CASES run all of them, so that both sides of every lane boundary are non-zero in some row of a case at every d2
  (asserted in tests/test_fastfood_wide_host.py).
* d2^-1.5 is a power of two at d2 = 1024 and 4096: VX is compared bit for bit there, to one ulp at 512 and 2048.
* One `int_chain` call per d2 -- the rows of all its shapes stacked, x zero beyond a shape's d, 5 blocks -- serves every case
  of that block size: rows and blocks are independent, so a case compares against a slice.
"""
import ctypes
import functools
from types import SimpleNamespace

import numpy as np

import test_gpu_fastfood_exact as ex
from test_gpu_fastfood_exact import (EXACT, NP, PHI_F32_BOUND, PHI_F64_BOUND, SENTINEL, _case, _exact_cos_sin, dyadic_S,
                                     int_chain, width_of)

D2S = (512, 1024, 2048, 4096)
POW2_NORM = (1024, 4096)  # d2^-1.5 is a power of two
FAMILY = "rr_fastfood64_kernel"
NMAX, KMAX = 37, 5
NNZ = 64


# ---- the instance table ---------------------------------------------------------------------------------------------------
def instance(compute, d2, d, k, ldx, ldo, x_align, out_align, mode):
    """(family, R, VEC, FULL) of the kernel ff_launch runs on a wide handle: R = d2 / 64 registers per lane, VEC = rows, row
    widths and both pointers fit vectors of vw = 16 bytes of the compute type (the conditions of the 16-lane families).  FULL is
    None: one wave owns one block, so the family has no partial-wave instances.  The mixture mode is refused."""
    assert compute in ("f32", "f64") and d2 in D2S and 1 <= d <= d2 and k >= 1
    if mode == "gm":
        raise ValueError("RR_ERR_UNSUPPORTED")
    assert mode in ("vx", "phi")
    vw = 4 if compute == "f32" else 2
    vec = ldx % vw == 0 and ldo % vw == 0 and d % vw == 0 and x_align % vw == 0 and out_align % vw == 0
    return (FAMILY, d2 // 64, vec, None)


def ident(inst, mode):
    """The identifier the bounds-checking build counts a launch of this instance under."""
    fam, R, vec, full = inst
    assert full is None
    return "%s/R%d/%s/%s" % (fam, R, mode, "vec" if vec else "scalar")


def all_idents():
    return [ident((FAMILY, R, v, None), mode) for R in (8, 16, 32, 64) for mode in ("vx", "phi") for v in (True, False)]


def reachable_instances():
    """Every register count in both launch variants and both modes (per arithmetic: the identifier does not name it)."""
    return {(compute, (FAMILY, R, v, None), mode) for compute in ("f32", "f64") for R in (8, 16, 32, 64) for v in (True, False)
            for mode in ("vx", "phi")}


def case_instance(c):
    w = width_of(c)
    return instance(c.compute, c.d2, c.d, c.k, c.d + c.ldx_extra, w + c.ldo_extra, c.x_off, c.out_off, c.mode)


# ---- data -------------------------------------------------------------------------------------------------------------------
def lane_boundaries(d):
    """(columns non-zero in every row, the lane boundaries b -- multiples of 2 -- not already among them)."""
    fixed = {0, d - 1}
    for b in range(256, d, 256):
        fixed |= {b - 1, b}
    assert len(fixed) <= 32
    return sorted(fixed), [b for b in range(2, d, 2) if b - 1 not in fixed and b not in fixed]


def shape_rows(d2, d):
    """Rows of a shape's data: NMAX, or at d = d2 as many as deal every lane boundary once, 16 a row."""
    return max(NMAX, -(-len(lane_boundaries(d)[1]) // 16)) if d == d2 else NMAX


def nonzero_columns(d, n_rows, seed):
    """(n_rows, <= NNZ) column indices, -1 padded: see the module docstring."""
    fixed, bounds = lane_boundaries(d)
    np.random.RandomState(seed).shuffle(bounds)
    out = -np.ones((n_rows, NNZ), dtype=np.int64)
    for r in range(n_rows):
        cols = list(fixed)
        for i in range(16):
            b = bounds[(r * 16 + i) % len(bounds)]
            cols += [b - 1, b]
        cols = sorted(set(cols))
        out[r, :len(cols)] = cols
    return out


def shape_dims(d2):
    """The input widths that have cases at this block size."""
    return (d2, d2 - 1, d2 // 2 + 1) + ((d2 // 2 + 4,) if d2 != 4096 else ())


@functools.lru_cache(maxsize=None)
def block_data(d2):
    """Integer data and reference of every shape of a block size, KMAX blocks: x in [-3, 3] \\ {0} on at most 64 columns per
    row, 1 / l in {1, 2, 4} per dimension (a shape of width d takes the first d), B = +-1, G in [-3, 3], PI a permutation per
    block, integer S in [1, 4] for VX.  The rows of all shapes go through ONE int_chain call (its +-1 Hadamard matrix takes
    seconds to build at d2 = 4096), each padded with zeros to d2 columns, which is what the chain does with a narrower x."""
    rs = np.random.RandomState(d2 * 7)
    inv_ls = rs.choice([1, 2, 4], size=d2)
    B = rs.randint(2, size=(KMAX, d2)) * 2 - 1
    G = rs.randint(-3, 4, size=(KMAX, d2))
    PI = np.array([rs.permutation(d2) for _ in range(KMAX)])
    S_int = rs.randint(1, 5, size=(KMAX, d2)).astype(np.float64)
    Xs, nzs = {}, {}
    for d in shape_dims(d2):
        n_rows = shape_rows(d2, d)
        X = np.zeros((n_rows, d2), dtype=np.int64)
        nz = nonzero_columns(d, n_rows, d2 + d)
        for r in range(n_rows):
            cols = nz[r][nz[r] >= 0]
            X[r, cols] = rs.choice([-3, -2, -1, 1, 2, 3], size=len(cols))
        Xs[d], nzs[d] = X, nz
    stacked = np.concatenate([Xs[d] for d in shape_dims(d2)])
    I, A = int_chain(stacked, inv_ls, B, G, PI, blas=d2 >= 2048)
    assert (np.abs(stacked) * inv_ls).sum(axis=1).max() <= 768 and np.all(np.abs(I) <= A)
    out, r0 = {}, 0
    for d in shape_dims(d2):
        n_rows = Xs[d].shape[0]
        assert not Xs[d][:, d:].any()
        F = SimpleNamespace(X=Xs[d][:, :d].copy(), inv_ls=inv_ls[:d].copy(), B=B, G=G, PI=PI, S_int=S_int, I=I[r0:r0 + n_rows],
                            A=A[r0:r0 + n_rows], nz=nzs[d])
        for a in vars(F).values():
            a.setflags(write=False)
        out[d] = F
        r0 += n_rows
    return out


def shape_data(d2, d):
    return block_data(d2)[d]


def case_data(c):
    """The slice of the shape's data a case runs on, its S (integers, + 2^-30 under sfrac, for VX; the dyadic constant for
    features) and its exactness bound, asserted."""
    assert c.k <= KMAX and c.ard
    F = shape_data(c.d2, c.d)
    w = c.k * c.d2
    rows = np.arange(c.N) % F.X.shape[0]  # (more rows than the shape has -- the chunk-seam case -- repeat them)
    I, A = F.I[rows, :w], F.A[rows, :w]
    assert A.max() < EXACT[c.compute], (c.label, int(A.max()))
    S = (F.S_int[:c.k] + (2.0 ** -30 if c.sfrac else 0.0)) if c.mode == "vx" else np.full((c.k, c.d2), dyadic_S(c.d2)[0])
    return SimpleNamespace(X=F.X[rows], ls=1.0 / F.inv_ls, B=F.B[:c.k], G=F.G[:c.k], PI=F.PI[:c.k], S=S, I=I, A=A)


# ---- cases ------------------------------------------------------------------------------------------------------------------
def grid_cases():
    """Every d2 in both arithmetics and both modes through the host-buffer calls: d = d2 (vector accesses), d2 - 1 and d2 / 2 + 1
    (odd: the scalar variant, the second with whole register groups beyond d), d2 / 2 + 4 (vector accesses with lanes and
    groups beyond d: the clamped loads); k = 1, 3, 4, 5 and N = 1, 2, 7, 37 dealt over them (N = 1, 2: fewer rows than the
    workgroup has waves; 37 = 9 x 4 + 1: a ragged last round)."""
    out = []
    for compute in ("f32", "f64"):
        for d2 in D2S:
            for d, k, N in ((d2, 4, 7), (d2 - 1, 3, 2), (d2 // 2 + 1, 1, 1), (d2, 5, 37), (d2 // 2 + 4, 3, 7)):
                if d2 == 4096 and d == d2 // 2 + 4:
                    continue  # (one reference less at the costliest size; 2048 / 2 + 4 runs the same code at R = 32)
                for mode in ("vx", "phi"):
                    out.append(_case("wide/%s/d2=%d/d=%d/k=%d/N=%d/%s" % (compute, d2, d, k, N, mode), compute, d2, d, k, N, mode))
    return out


def variant_cases():
    """Device-resident calls whose leading dimensions or pointers flip VEC on their own; sentinel-filled output buffers."""
    out = []
    flips = [("aligned", {}), ("ldx+1", {"ldx_extra": 1}), ("ldo+1", {"ldo_extra": 1}), ("ldo+4", {"ldo_extra": 4}),
             ("x+1", {"x_off": 1}), ("out+1", {"out_off": 1})]
    for compute in ("f32", "f64"):
        for d2 in D2S:
            for name, kw in flips:
                out.append(_case("wide/dev/%s/d2=%d/%s" % (compute, d2, name), compute, d2, d2, 3, 7, "phi", api="dev", **kw))
    out.append(_case("wide/dev/f32/x=f64/o=f64/out+1", "f32", 512, 512, 3, 7, "phi", api="dev", xdt="f64", odt="f64", out_off=1))
    out.append(_case("wide/dev/f64/x=f32/o=f32/ldo+2", "f64", 512, 512, 3, 7, "phi", api="dev", xdt="f32", odt="f32", ldo_extra=2))
    return out


def dtype_cases():
    """All eight x_dtype x compute x out_dtype combinations of ff_dispatch at d2 = 512, VX a second time with S = integer + 2^-30
    (see tests/test_gpu_fastfood_exact.py: a float32 table or route then shows in a float64 output)."""
    out = []
    for xdt in ("f32", "f64"):
        for compute in ("f32", "f64"):
            for odt in ("f32", "f64"):
                for mode in ("vx", "phi"):
                    out.append(_case("wide/dtype/x=%s/c=%s/o=%s/%s" % (xdt, compute, odt, mode), compute, 512, 512, 3, 7, mode,
                                     xdt=xdt, odt=odt))
                out.append(_case("wide/dtype/x=%s/c=%s/o=%s/vx+2^-30" % (xdt, compute, odt), compute, 512, 512, 3, 7, "vx",
                                 xdt=xdt, odt=odt, sfrac=True))
    return out


def cover_cases():
    """Every row of the shapes d = d2 at the two block sizes where that is more than 37: over a case's rows both sides of every
    lane boundary carry a non-zero.  k = 1; VX and features in float32, VX in float64."""
    return [_case("wide/cover/%s/d2=%d/N=%d/%s" % (compute, d2, shape_rows(d2, d2), mode), compute, d2, d2, 1, shape_rows(d2, d2), mode)
            for d2 in (2048, 4096) for compute, mode in (("f32", "vx"), ("f32", "phi"), ("f64", "vx"))]


GRID, VARIANTS, DTYPES, COVER_CASES = grid_cases(), variant_cases(), dtype_cases(), cover_cases()
ALL_CASES = GRID + VARIANTS + DTYPES + COVER_CASES
# rows per workgroup forced to 9 (RR_FF_ROWS_PER_BLOCK): N = 10 is one full workgroup -- whose waves take 3, 2, 2, 2 rows (5 and
# 4 in the two-wave instance), so the load of the next row's x behind the current one runs at every size -- plus one row
RP = 9
RP_CASES = [_case("wide/rp=9/%s/d2=%d/%s" % (compute, d2, mode), compute, d2, d2, 3, RP + 1, mode)
            for compute in ("f32", "f64") for d2 in D2S for mode in ("vx", "phi")]
# ff_host_call streams rows in chunks of 256 MiB / (bytes per row): d = 4096, k = 5 in float32 is 4 (4096 + 2 * 4096 * 5) =
# 180 224 bytes per row, 1489 rows per chunk -- 1497 rows cross one seam (the rows repeat with the period of the shape's data)
SEAM_CASE = _case("wide/seam", "f32", 4096, 4096, 5, 1497, "phi", xdt="f32", odt="f32")
SEAM_ROWS_PER_CHUNK = (256 << 20) // (4 * (4096 + 2 * 4096 * 5))


def run_and_check_seam():
    """The seam case: the rows of the shape's data through the exact check, every later row bit-identical to the row it repeats
    (the same integers through the same kernel: any difference is a misplaced or torn row)."""
    c = SEAM_CASE
    P = shape_rows(c.d2, c.d)
    assert SEAM_ROWS_PER_CHUNK == 1489 and P < SEAM_ROWS_PER_CHUNK < c.N
    D = case_data(c)
    got = run_case(c, D).view(np.uint32)
    head = c._replace(N=P)
    check_phi(head, case_data(head), got[:P].view(np.float32))
    for r0 in range(P, c.N, P):
        m = min(P, c.N - r0)
        assert np.array_equal(got[r0:r0 + m], got[:m]), "rows %d..%d differ from the rows they repeat" % (r0, r0 + m)


def ids(cases):
    return [c.label for c in cases]


# ---- running a case and checking it -----------------------------------------------------------------------------------------
def handle(c, D):
    from revrand_amd import _hip
    return _hip.FastFoodHandle(c.d, c.d2, c.k, D.B, D.G, D.PI, D.S, compute=c.compute, wide=True)


def run_case(c, D):
    """The case's output (N, width) in its output dtype.  Device-resident calls check on the way that every element of the
    sentinel-filled buffer outside the written block -- before an offset output, the columns beyond `width`, two rows beyond
    N -- still holds the sentinel."""
    ff = handle(c, D)
    X = D.X.astype(NP[c.xdt])
    odt = NP[c.odt]
    w = width_of(c)
    if c.api == "host":
        assert not (c.ldx_extra or c.ldo_extra or c.x_off or c.out_off)
        return ff.vx(X, D.ls, out_dtype=odt) if c.mode == "vx" else ff.transform(X, D.ls, out_dtype=odt)
    assert c.mode == "phi"
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
        ff.transform_dev(dX, D.ls, ctypes.c_void_p(bo.ptr.value + c.out_off * osz), out_dtype=odt, ldphi=ldo)
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


def check_vx(c, D, got):
    """VX = T(I) * T(S d2^-1.5), one multiply in the compute type, cast to the output type: bit for bit at d2 = 1024, 4096, where
    d2^-1.5 is a power of two; at 512 and 2048 within one ulp of the coarser of the two types (the library's pow() may round
    d2^-1.5 the other way)."""
    T, O = NP[c.compute], NP[c.odt]
    want_T = D.I.astype(T) * np.tile((D.S * float(c.d2) ** -1.5).astype(T).ravel(), (c.N, 1))
    want = want_T.astype(O)
    assert got.dtype == O and got.shape == want.shape
    if c.d2 in POW2_NORM:
        bad = got != want
        print("%-48s VX bit for bit: %d of %d differ" % (c.label, int(bad.sum()), bad.size))
        assert not bad.any(), "%s: %d of %d differ, max |diff| %g" % (c.label, int(bad.sum()), bad.size, np.abs(got - want).max())
    else:
        ulp = np.maximum(np.spacing(np.abs(want_T)).astype(np.float64), np.spacing(np.abs(want)).astype(np.float64))
        err = np.abs(got.astype(np.float64) - want.astype(np.float64)) / ulp
        print("%-48s VX max error %.2f ulp" % (c.label, err.max()))
        assert err.max() <= 1.0, (c.label, err.max())


def check_phi(c, D, got):
    """Features at exactly known phases.  float32: phase = I / 16 revolutions, exact, so PHI_F32_BOUND alone.  float64: the
    kernel's single multiply I * Srev64 (Srev64 ~1e-17 off 2^-4), reduced exactly; PHI_F64_BOUND, plus one ulp of pow() in
    Srev64 times the phase where d2^-1.5 is not a power of two, plus the output rounding of a float32 output."""
    n = c.d2 * c.k
    ph = D.I.astype(np.float64) / 16 if c.compute == "f32" else D.I.astype(np.float64) * dyadic_S(c.d2)[1]
    want = np.concatenate(_exact_cos_sin(ph), axis=1)
    assert got.dtype == NP[c.odt] and got.shape == want.shape == (c.N, 2 * n)
    if c.compute == "f32":
        b = np.full(ph.shape, PHI_F32_BOUND)
    else:
        b = np.full(ph.shape, PHI_F64_BOUND)
        if c.d2 not in POW2_NORM:
            b = b + 2 * np.pi * 2.0 ** -52 * np.abs(ph)
        if c.odt == "f32":
            b = b + 2.0 ** -24
    err = np.abs(got.astype(np.longdouble) * np.sqrt(np.longdouble(n)) - want).astype(np.float64)
    bound = np.tile(b, (1, 2))
    print("%-48s Phi max |error| %.3e (bound %.3e), max phase %.0f rev" % (c.label, err.max(), bound.min(), np.abs(ph).max()))
    assert np.all(err <= bound), "%s: %d of %d beyond the bound, max |error| %g" % (c.label, int((err > bound).sum()), err.size, err.max())


def run_and_check(c):
    D = case_data(c)
    got = run_case(c, D)
    (check_vx if c.mode == "vx" else check_phi)(c, D, got)
    return D, got


# ---- the feature matrix --------------------------------------------------------------------------------------------------
FEATMAT = [("f32", 512, 4 + 3), ("f64", 1024, 8)]  # (arithmetic of the basis, d2, col0): a misaligned and an aligned block


def run_featmat(compute, d2, col0):
    """rr_featmat_put_fastfood at a non-zero col0 behind a linear child: the block at the exactly known phases, every other
    column of the stored matrix bit-identical to its state before the call; returns the instance the table names."""
    from revrand_amd import _hip
    c = _case("wide/featmat/%s/d2=%d/col0=%d" % (compute, d2, col0), compute, d2, d2, 3, NMAX, "phi", xdt="f32", odt="f32")
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
    fm.put_fastfood(ff, dX, D.ls, col0)
    after = fm.download()
    inst = instance(compute, d2, d2, 3, d2, after.shape[1], 0, col0, "phi")
    check_phi(c, D, np.ascontiguousarray(after[:, col0:col0 + w]))
    keep = np.ones(after.shape[1], dtype=bool)
    keep[col0:col0 + w] = False
    assert np.array_equal(after.view(np.uint32)[:, keep], before[:, keep])
    assert np.all(after[:, F:] == 0)
    return inst


# ---- which instance ran (the bounds-checking build's launch counts) -------------------------------------------------------
def census_runs():
    """[(label, environment, run)]: every case that launches the wide kernel; run() returns the identifier the table names."""
    def of(c):
        def run():
            run_case(c, case_data(c))
            return ident(case_instance(c), c.mode)
        return run
    runs = [(c.label, {}, of(c)) for c in ALL_CASES]
    runs += [(c.label, {"RR_FF_ROWS_PER_BLOCK": str(RP)}, of(c)) for c in RP_CASES]
    runs.append((SEAM_CASE.label, {}, of(SEAM_CASE)))  # (two launches: one per chunk)
    for f in FEATMAT:
        runs.append(("wide/featmat/%s/d2=%d/col0=%d" % f, {}, lambda f=f: ident(run_featmat(*f), "phi")))
    return runs


def census():
    """Launches per instance of the wide family -- and of the narrow families, which must not run at all -- for every entry of
    census_runs, under a library that counts them (rr_debug_kernel_launches): [(label, {identifier: launches}, identifier the
    table names)]."""
    import os
    from revrand_amd import _hip
    dev = _hip.get_device()
    lib = dev.lib
    assert lib.rr_debug_kernel_launches(None) == 0
    names = all_idents() + ex.all_idents()
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
