"""FastFoodRBF / FastFoodGM children of the float64 feature matrix (rr_featmat64_put_fastfood[_gm], rr_featmat64_pass2_xt /
_glm_xt; docs/KERNELS.md 3.49).

1. What `put` writes: the exact-phase data of tests/test_gpu_fastfood_exact.py / tests/fastfood_wide_cases.py through the matrix,
   the block within PHI_F64_BOUND whatever the handle's own arithmetic, every other element of a sentinel-prefilled matrix
   untouched; the mixture mode also against the reference's recorded features.
2. The contraction T = X^T A on integers: `==` against NumPy, against pass2_rff / glm_rff with a dense handle up to 128
   columns, one row slab against three above.
3. `_elbo` of StandardLinearModel(resident_bases="all") against the oracle at the float64 state's tolerances.
4. The float64 GLM step and a seeded 20-step fit against the oracle.
Figures are printed (run with -s)."""
import numpy as np
import pytest

import fastfood_wide_cases as wide
import glm_f64_cases as gc
import revrand_oracle as orc
import test_gpu_fastfood_exact as ex
import test_gpu_glm_f64 as g64
from conftest import normwise
from test_gpu_fastfood_exact import INV2PI, PHI_F64_BOUND, SENTINEL, U
from test_gpu_fastfood_gm_wide import _dot_bound, _gm
from test_gpu_fastfood_wide import _phase_bound

pytestmark = pytest.mark.gpu

SENT64 = np.array([SENTINEL[8]], dtype=np.uint64).view(np.float64)[0]   # a finite double no feature can equal
COL0S = (4, 4 + 3)   # aligned (vector stores) and odd (the kernels' scalar-store instances)


# ---- 1: what put writes ----------------------------------------------------------------------------------------------------------
PUT_SHAPES = [(d2, k, rows) for d2 in (8, 16, 64, 256, 512, 4096) for k in ((1, 3) if d2 != 4096 else (1,)) for rows in (1, 17)]


def _put_case(d2, k, rows, mode="phi"):
    """(case, data, handle factory, checker) on the exact-phase data of the block size's own test module, float64 phases."""
    if d2 >= 512:
        c = wide._case("f64put/wide/d2=%d/k=%d/N=%d" % (d2, k, rows), "f64", d2, d2, k, rows, mode)
        D = wide.case_data(c)
        return c, D, (lambda compute: _handle(c, D, compute, True)), wide.check_phi
    d = d2 if k == 1 else d2 - 1
    c = ex._case("f64put/d2=%d/k=%d/N=%d/%s" % (d2, k, rows, mode), "f64", d2, d, k, rows, mode)
    D = ex.case_data(c)
    return c, D, (lambda compute: _handle(c, D, compute, False)), ex.check_phi


def _handle(c, D, compute, wide_handle):
    from revrand_amd import _hip
    return _hip.FastFoodHandle(c.d, c.d2, c.k, D.B, D.G, D.PI, D.S, compute=compute, wide=wide_handle)


def _put_and_check(c, D, ff, check, xdt, col0, put):
    """One put into a matrix whose every element of [0, F) holds the sentinel: the block checked, the rest compared bit for bit
    with the matrix before the call (sentinels in [0, F), the zero padding beyond)."""
    from revrand_amd import _hip
    w = ex.width_of(c)
    F = col0 + w + 5
    fm = _hip.FeatureMatrix64(c.N, F)
    fm.begin(c.N)
    fm.put_host(np.full((c.N, F), SENT64), 0)
    before = fm.download().view(np.uint64).copy()
    assert np.all(before[:, :F] == SENTINEL[8]) and not before[:, F:].any()
    fm.begin(c.N)   # (forgets the claimed columns, leaves the data rows alone)
    dX = ff.dev.upload_matrix(np.ascontiguousarray(D.X.astype(ex.NP[xdt])))
    try:
        put(fm, dX, col0)
        after = fm.download()
    finally:
        dX.free()
    check(c, D, np.ascontiguousarray(after[:, col0:col0 + w]))
    keep = np.ones(after.shape[1], dtype=bool)
    keep[col0:col0 + w] = False
    assert np.array_equal(after.view(np.uint64)[:, keep], before[:, keep]), "%s: elements outside the block were written" % c.label


@pytest.mark.parametrize("d2,k,rows", PUT_SHAPES, ids=["d2=%d-k=%d-rows=%d" % s for s in PUT_SHAPES])
def test_put_fastfood_writes_float64_features_and_nothing_else(d2, k, rows):
    c, D, make, check = _put_case(d2, k, rows)
    for compute in ("f32", "f64"):      # the handle's own arithmetic: the matrix runs the float64 instance either way
        ff = make(compute)
        for xdt in ("f32", "f64"):
            for col0 in COL0S:
                _put_and_check(c._replace(label="%s/h=%s/x=%s/col0=%d" % (c.label, compute, xdt, col0)), D, ff, check, xdt, col0,
                               lambda fm, dX, c0: fm.put_fastfood(ff, dX, D.ls, c0))


@pytest.mark.parametrize("d2,k,rows", [(16, 1, 1), (16, 3, 17), (256, 1, 17), (256, 3, 1)])
def test_put_fastfood_gm_writes_float64_features_and_nothing_else(d2, k, rows):
    c, D, make, check = _put_case(d2, k, rows, mode="gm")
    for compute in ("f32", "f64"):
        ff = make(compute)
        for xdt in ("f32", "f64"):
            for col0 in COL0S:
                _put_and_check(c._replace(label="%s/h=%s/x=%s/col0=%d" % (c.label, compute, xdt, col0)), D, ff, check, xdt, col0,
                               lambda fm, dX, c0: fm.put_fastfood_gm(ff, dX, D.mean, D.ls, c0))


def _gm_against_golden(b, X, mean, ls, want, cols, m_dot, label):
    """The four blocks of put_fastfood_gm (both handle arithmetics, both X types, both offsets) against the reference's recorded
    Phi, element by element, at the float64 bound of tests/test_gpu_fastfood_gm_wide.py::test_transform_against_the_recorded_reference:
        2 pi (chain(u64) + chain(u64) + dot(u64, m_dot) + dot(u64, d) + u64 (A + sum |x_i mean_i| / 2 pi)) + PHI_F64_BOUND + 1e-15"""
    from revrand_amd import _hip
    u = U["f64"]
    chain = _phase_bound(b, X, ls, u)
    A = chain / float(np.expm1((2 * int(np.log2(b.d2)) + 7) * np.log1p(u)))
    sxm = (np.abs(X) * np.abs(mean) * INV2PI).sum(axis=1)[:, None]
    ph = 2 * chain + _dot_bound(X, mean, u, m_dot) + _dot_bound(X, mean, u, X.shape[1]) + u * (A + sxm)
    bound = np.tile(2 * np.pi * ph + PHI_F64_BOUND + 1e-15, (1, 4))[:, cols]
    N, w = X.shape[0], 4 * b.n
    worst = 0.0
    for compute in ("f32", "f64"):
        ff = _hip.FastFoodHandle(b.d, b.d2, b.k, b.B, b.G, b.PI, b.S, compute=compute, wide="gm")
        for xdt in (np.float32, np.float64):
            if not np.array_equal(X.astype(xdt).astype(np.float64), X):
                continue   # (the recorded X is not float32 data: float64 rows only)
            for col0 in COL0S:
                F = col0 + w + 5
                fm = _hip.FeatureMatrix64(N, F)
                fm.begin(N)
                fm.put_host(np.full((N, F), SENT64), 0)
                fm.begin(N)
                dX = ff.dev.upload_matrix(np.ascontiguousarray(X.astype(xdt)))
                try:
                    fm.put_fastfood_gm(ff, dX, mean, ls, col0)
                    got = fm.download()
                finally:
                    dX.free()
                keep = np.ones(got.shape[1], dtype=bool)
                keep[col0:col0 + w] = False
                assert np.all(got.view(np.uint64)[:, keep][:, :F - w] == SENTINEL[8]) and not got[:, F:].any()
                err = np.abs(got[:, col0:col0 + w][:, cols] - want) * np.sqrt(2 * b.n)
                worst = max(worst, float((err / bound).max()))
                assert np.all(err <= bound), (label, compute, xdt, col0, float((err / bound).max()))
    print("%s: put_fastfood_gm against the recorded reference, max error / bound %.3f (smallest bound %.2e)" % (label, worst, bound.min()))


def test_put_fastfood_gm_against_the_recorded_reference_at_d2_16(golden):
    import revrand_amd.basis_functions as bs
    from revrand_amd.btypes import Bound, Parameter, Positive
    g = golden("fastfood_gm")
    d, nb, seed = 16, 32, 3   # (tests/test_gpu_fastfood.py::test_fastfood_gm_golden's case)
    b = bs.FastFoodGM(nbases=nb, Xdim=d, random_state=seed, mean=Parameter(np.zeros(d), Bound()),
                      lenscale=Parameter(np.ones(d), Positive()), dtype="f64")
    X, mean, ls = g["d16_nb32_X"], g["d16_nb32_mean"], g["d16_nb32_ls"]
    # the lane-major kernel's reduction of mX: at most d additions on a path whatever its order, the product and the table's
    # conversion -- d + 2 roundings
    _gm_against_golden(b, X, mean, ls, g["d16_nb32_Phi"], np.arange(4 * b.n), d + 2, "d2=16")


def test_put_fastfood_gm_against_the_recorded_reference_on_a_wide_handle(golden):
    g = golden("fastfood_gm_wide")
    d, nb = 300, 600   # (GOLDEN_SHAPES[0] of tests/test_gpu_fastfood_gm_wide.py: d2 = 512)
    b = _gm(d, nb, "f64")
    X, cols, mean, ls = g["X_d300"].astype(np.float64), g["cols_d300"], g["mean_d300"], g["ls_ard_d300"]
    _gm_against_golden(b, X, mean, ls, g["Phi_d300"], cols, b.d2 // 64 + 8, "d2=512 (wide_gm)")


def test_put_refusals():
    from revrand_amd import _hip
    rs = np.random.RandomState(0)
    B, G, PI, S = orc.fastfood_matrices(8, 5, 0)      # d2 = 8: below the mixture mode
    narrow = _hip.FastFoodHandle(5, 8, 1, B, G, PI, S, compute="f64")
    Bw, Gw, PIw, Sw = orc.fastfood_matrices(512, 300, 0)
    plain_wide = _hip.FastFoodHandle(300, 512, 1, Bw, Gw, PIw, Sw, compute="f64", wide=True)
    fm = _hip.FeatureMatrix64(4, 40)
    fm.begin(4)
    dX = narrow.dev.upload_matrix(rs.randn(4, 5))
    dXw = narrow.dev.upload_matrix(rs.randn(4, 300))
    with pytest.raises(_hip.HipError) as e:
        fm.put_fastfood_gm(narrow, dX, np.zeros(5), np.ones(5), 0)
    assert e.value.code == -5
    with pytest.raises(_hip.HipError) as e:
        fm.put_fastfood_gm(plain_wide, dXw, np.zeros(300), np.ones(300), 0)
    assert e.value.code in (-1, -5)   # (columns out of range comes first on a 40-column matrix)
    big = _hip.FeatureMatrix64(4, 4 * 512)
    big.begin(4)
    with pytest.raises(_hip.HipError) as e:
        big.put_fastfood_gm(plain_wide, dXw, np.zeros(300), np.ones(300), 0)
    assert e.value.code == -5
    big.put_host(np.zeros((4, 4 * 512)), 0)   # nothing was claimed by the refused call
    with pytest.raises(_hip.HipError) as e:
        fm.put_fastfood(narrow, dX, 1.0, 40 - 15)      # 16 columns do not fit
    assert e.value.code == -1
    fm.put_fastfood(narrow, dX, 1.0, 3)
    with pytest.raises(_hip.HipError) as e:
        fm.put_fastfood(narrow, dX, 1.0, 10)           # overlaps the block just written
    assert e.value.code == -1
    dX.free()
    dXw.free()


# ---- 2: the contraction, exactly ---------------------------------------------------------------------------------------------------
XT_D = (1, 5, 100, 128, 129, 130, 300, 513)
XT_N = (16, 130)
XT_ROWS = (1, 17, 500)
XT_COL0 = 3
GAUSSIAN = 2   # RR_LIK_GAUSSIAN


def _xt_case(rows, n, d, glm):
    """Integer P, m, C, y, X sized as tests/test_gpu_pass2_exact.py::_case64, every sum an integer below 2^53 (asserted); glm: the
    EdPhi of a one-sample Gaussian step of unit variance, (y - P w) w^T.  Returns (P, m, C, y, X, w, T)."""
    rs = np.random.RandomState((rows * 131 + n * 17 + d) * 2 + int(glm))
    F = XT_COL0 + 2 * n + 2
    P = rs.randint(-1000, 1001, size=(rows, F)).astype(np.float64)
    m = rs.randint(-10, 11, size=F).astype(np.float64)
    up = np.triu(rs.randint(-10, 11, size=(F, F)).astype(np.float64), 1)
    C = up + up.T + np.diag(rs.randint(1, 11, size=F).astype(np.float64))
    y = rs.randint(-1000, 1001, size=rows).astype(np.float64)
    X = rs.randint(-100, 101, size=(rows, d)).astype(np.float64)
    w = rs.randint(-10, 11, size=F).astype(np.float64)
    c0 = XT_COL0
    Pc, Ps = P[:, c0:c0 + n], P[:, c0 + n:c0 + 2 * n]
    if glm:
        E = (y - P @ w)[:, None] * w[None, :]
        Ec, Es = E[:, c0:c0 + n], E[:, c0 + n:c0 + 2 * n]
        A, W = Es * Pc - Ec * Ps, np.abs(Es * Pc) + np.abs(Ec * Ps)
        big = max((np.abs(P) @ np.abs(w)).max() + 1000, np.abs(E).max())
    else:
        U_, err = P @ C, y - P @ m
        Uc, Us = U_[:, c0:c0 + n], U_[:, c0 + n:c0 + 2 * n]
        mc, ms = m[c0:c0 + n], m[c0 + n:c0 + 2 * n]
        A = err[:, None] * (Pc * ms - Ps * mc) - (Pc * Us - Ps * Uc)
        W = np.abs(err)[:, None] * (np.abs(Pc) * np.abs(ms) + np.abs(Ps) * np.abs(mc)) + np.abs(Pc * Us) + np.abs(Ps * Uc)
        big = max((np.abs(P) @ np.abs(C)).max(), (np.abs(P) @ np.abs(m)).max() + 1000, (err * err).sum())
    big = max(big, (np.abs(X).T @ W).max())
    assert (1 << 24) < big < 2.0 ** 53, big     # exact in float64 in any order, out of reach of any float32 step
    return P, m, C, y, X, w, X.T @ A


def _run_xt(fm, dev, P, m, C, y, w, glm):
    """Fill the matrix and run the pass that leaves what the contraction reads."""
    rows = P.shape[0]
    fm.begin(rows)
    fm.put_host(P, 0)
    dy = dev.upload_vector(y)
    try:
        if glm:
            fm.glm_step(dy, None, GAUSSIAN, 1.0, w[None, :], 1, 1)
        else:
            fm.pass2_begin(m, C)
            fm.pass2_rows(dy)
    finally:
        dev.sync()
        dy.free()


def _contract(fm, dev, X, xdt, d, n, glm, rff=None):
    from revrand_amd import _hip
    if rff is None:
        ld = _hip.xt_padded_dim(d)
        dX = dev.upload_matrix(np.ascontiguousarray(X.astype(xdt)), ld_dev=ld + (ld & 1))
    else:
        dX = rff.upload(np.ascontiguousarray(X.astype(xdt)))
    dT = dev.zeros(d * n * 8)
    try:
        if rff is None:
            (fm.glm_xt if glm else fm.pass2_xt)(dX, d, n, XT_COL0, dT)
        else:
            (fm.glm_rff if glm else fm.pass2_rff)(rff, dX, XT_COL0, dT)
        return dev.download(dT, (d, n), np.float64)
    finally:
        dX.free()
        dT.free()


@pytest.mark.parametrize("glm", [False, True], ids=["pass2_xt", "glm_xt"])
@pytest.mark.parametrize("n", XT_N)
@pytest.mark.parametrize("d", XT_D)
def test_the_contraction_is_exact(d, n, glm, monkeypatch):
    from revrand_amd import _hip
    dev = _hip.get_device()
    rff = _hip.RffHandle(np.random.RandomState(d).randn(d, n), compute="f64") if d <= 128 else None
    for rows in XT_ROWS:
        P, m, C, y, X, w, T = _xt_case(rows, n, d, glm)
        fm = _hip.FeatureMatrix64(rows, P.shape[1])
        _run_xt(fm, dev, P, m, C, y, w, glm)
        for det in (False, True):
            with g64._Deterministic(det):
                for xdt in (np.float32, np.float64):
                    what = "%s rows=%d n=%d d=%d det=%s x=%s" % ("glm_xt" if glm else "pass2_xt", rows, n, d, det, np.dtype(xdt).name)
                    got = _contract(fm, dev, X, xdt, d, n, glm)
                    assert np.array_equal(got, T), (what, int((got != T).sum()), float(np.abs(got - T).max()))
                    if rff is not None:
                        assert np.array_equal(_contract(fm, dev, X, xdt, d, n, glm, rff=rff), got), what + ": differs from _rff"
        if d > 128:
            # the row slabs: one (forced) against three on the same integers, and a second call adds to dT
            for slabs in ("1", "3"):
                monkeypatch.setenv("RR_GLM64_KSLABS", slabs)
                got = _contract(fm, dev, X, np.float64, d, n, glm)
                assert np.array_equal(got, T), ("slabs=" + slabs, rows, n, d)
            monkeypatch.delenv("RR_GLM64_KSLABS")


@pytest.mark.parametrize("glm", [False, True], ids=["pass2_xt", "glm_xt"])
def test_the_wide_contraction_repeats_bit_for_bit_on_real_data(glm):
    """Non-integer data, d = 300: two runs give the same bits in the default mode (no atomics on this route), and the result is
    the float64 product to rounding."""
    from revrand_amd import _hip
    dev = _hip.get_device()
    rs = np.random.RandomState(4)
    rows, n, d = 500, 130, 300
    F = XT_COL0 + 2 * n + 2
    P, m, y, X, w = rs.randn(rows, F), rs.randn(F), rs.randn(rows), rs.randn(rows, d), 0.1 * rs.randn(F)
    C = rs.randn(F, F)
    C = C @ C.T / F
    fm = _hip.FeatureMatrix64(rows, F)
    _run_xt(fm, dev, P, m, C, y, w, glm)
    a, b = (_contract(fm, dev, X, np.float64, d, n, glm) for _ in range(2))
    assert np.array_equal(a, b)
    c0 = XT_COL0
    Pc, Ps = P[:, c0:c0 + n], P[:, c0 + n:c0 + 2 * n]
    if glm:
        E = (y - P @ w)[:, None] * w[None, :]
        A = E[:, c0 + n:c0 + 2 * n] * Pc - E[:, c0:c0 + n] * Ps
    else:
        U_, err = P @ C, y - P @ m
        A = err[:, None] * (Pc * m[c0 + n:c0 + 2 * n] - Ps * m[c0:c0 + n]) - (Pc * U_[:, c0 + n:c0 + 2 * n] - Ps * U_[:, c0:c0 + n])
    print("wide contraction on real data (%s): normwise %.2e" % ("glm" if glm else "pass2", normwise(a, X.T @ A)))
    assert normwise(a, X.T @ A) < 1e-12


def test_contraction_refusals_are_error_codes_before_any_launch():
    from revrand_amd import _hip
    dev = _hip.get_device()
    rs = np.random.RandomState(1)
    rows, n, d = 17, 16, 5
    F = 2 * n + 3
    fm = _hip.FeatureMatrix64(rows, F)
    P, m, C, y = rs.randn(rows, F), rs.randn(F), np.eye(F), rs.randn(rows)
    dX = dev.upload_matrix(rs.randn(rows, d), ld_dev=8)
    dXw = dev.upload_matrix(rs.randn(rows, 200), ld_dev=200)
    dT = dev.zeros(4096 * n * 8)
    null = _hip.DeviceView(dX, 0, rows)
    null.ptr = _hip.ctypes.c_void_p(None)

    def refused(call, *args):
        with pytest.raises(_hip.HipError) as e:
            call(*args)
        assert e.value.code == -1, e.value
    fm.begin(rows)
    fm.put_host(P, 0)
    refused(fm.pass2_xt, dX, d, n, 0, dT)         # no pass2_rows
    refused(fm.glm_xt, dX, d, n, 0, dT)           # no step
    fm.pass2_begin(m, C)
    refused(fm.pass2_xt, dX, d, n, 0, dT)         # pass2_begin alone
    dy = dev.upload_vector(y)
    fm.pass2_rows(dy)
    refused(fm.glm_xt, dX, d, n, 0, dT)           # rows, but no step since
    refused(fm.pass2_xt, dX, d, n, F - 2 * n + 1, dT)   # columns out of range
    refused(fm.pass2_xt, dX, d, n, -1, dT)
    refused(fm.pass2_xt, dX, 4097, n, 0, dT)      # d > 4096
    refused(fm.pass2_xt, dX, 0, n, 0, dT)
    refused(fm.pass2_xt, dX, 9, n, 0, dT)         # ldx = 8 < the 16 the register kernel reads for d = 9
    refused(fm.pass2_xt, dXw, 201, n, 0, dT)      # ldx < d on the wide route
    refused(fm.pass2_xt, null, d, n, 0, dT)       # null X
    fm.pass2_xt(dX, d, n, 0, dT)                  # (and the matrix still serves the call)
    fm.glm_step(dy, None, GAUSSIAN, 1.0, rs.randn(1, F), 1, 1)
    refused(fm.pass2_xt, dX, d, n, 0, dT)         # a step since pass2_rows
    refused(fm.glm_xt, dX, d, n, F - 2 * n + 1, dT)
    refused(fm.glm_xt, dX, 4097, n, 0, dT)
    refused(fm.glm_xt, null, d, n, 0, dT)
    fm.glm_xt(dX, d, n, 0, dT)
    fm.begin(rows)
    refused(fm.glm_xt, dX, d, n, 0, dT)           # begin() forgets the step
    dev.sync()
    for buf in (dX, dXw, dT, dy):
        buf.free()


# ---- 3: _elbo end to end --------------------------------------------------------------------------------------------------------
def _slm_imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd.btypes import Bound, Parameter, Positive
    from revrand_amd.slm import StandardLinearModel
    return bs, Parameter, Positive, Bound, StandardLinearModel


def _no_host_features(monkeypatch, bs):
    def boom(*a, **k):
        raise AssertionError("the resident float64 fit called the basis' transform / grad")
    for cls in (bs.FastFoodRBF, bs.FastFoodGM):
        monkeypatch.setattr(cls, "transform", boom)
        monkeypatch.setattr(cls, "grad", boom)


def _slices3(g):
    return [g] if g.ndim == 2 else [g[:, :, i] for i in range(g.shape[2])]


def _check_elbo(slm, X, y, var, regs, hyp, o, want_h, label):
    nelbo, (ndvar, ndreg, ndhyp) = slm._elbo(X, y, var, regs, hyp)
    C = slm._state.best_covariance() if slm._state.best_on_device else slm.covariance_
    got_h = np.concatenate([np.atleast_1d(np.asarray(h, dtype=float)) for h in (ndhyp if isinstance(ndhyp, list) else [ndhyp])])
    errs = {"elbo": abs(-nelbo - o["elbo"]) / abs(o["elbo"]), "m": normwise(slm.weights_, o["m"]), "C": normwise(C, o["C"]),
            "dvar": abs(-ndvar - o["dvar"]) / abs(o["dvar"]), "dreg": normwise(-np.atleast_1d(ndreg), np.atleast_1d(o["dreg"])),
            "dhyp": normwise(-got_h, want_h)}
    print("float64 _elbo %-34s %s" % (label, {k: "%.2e" % v for k, v in errs.items()}))
    assert errs["elbo"] < 1e-9 and errs["m"] < 1e-6 and errs["C"] < 1e-6, (label, errs)
    assert errs["dvar"] < 1e-7 and errs["dreg"] < 1e-7 and errs["dhyp"] < 1e-6, (label, errs)


@pytest.mark.parametrize("ard", [False, True], ids=["iso", "ard"])
@pytest.mark.parametrize("d", [5, 20])
def test_elbo_of_a_concatenation_with_a_float64_fastfood_child(d, ard, monkeypatch):
    bs, Parameter, Positive, Bound, SLM = _slm_imports()
    rs = np.random.RandomState(7 + d)
    N = 333
    X = rs.randn(N, d)
    y = np.sin(X @ rs.randn(d)) + 0.1 * rs.randn(N)
    lsp = Parameter(np.ones(d), Positive()) if ard else Parameter(1.0, Positive())
    ff = bs.FastFoodRBF(nbases=40 if d == 5 else 70, Xdim=d, random_state=3, lenscale=lsp, dtype="f64")
    rbf = bs.RandomRBF(nbases=20, Xdim=d, random_state=4, lenscale=Parameter(1.0, Positive()), dtype="f64")
    cat = ff + bs.LinearBasis(onescol=True) + rbf
    ls0 = np.linspace(0.8, 1.4, d) if ard else 1.2
    ls2 = 1.3
    mats = (ff.B, ff.G, ff.PI, ff.S)
    blocks = [orc.fastfood_transform(X, *mats, ls0), orc.linear_transform(X, True), orc.rff_transform(X, rbf.W, ls2)]
    Phi = np.hstack(blocks)
    grads = [_slices3(orc.fastfood_grad(X, *mats, ls0)), [], _slices3(orc.rff_grad(X, rbf.W, ls2))]
    slabs = g64._pad_slabs(Phi, blocks, grads)
    e = np.cumsum([0] + [b.shape[1] for b in blocks])
    regs, var = [1.5, 0.7, 1.1], 0.3
    rd = np.concatenate([np.full(e[i + 1] - e[i], regs[i]) for i in range(3)])
    o = orc.slm_elbo(Phi, y, var, rd, [slice(e[i], e[i + 1]) for i in range(3)], slabs)
    # the default keyword keeps the parent's answer: the concatenation declines, the estimator takes transform / grad
    assert SLM(cat)._make_state(X, y) is None
    _no_host_features(monkeypatch, bs)
    for chunk in (None, 84):
        slm = SLM(cat, resident_bases="all")
        slm.obj_ = -np.inf
        st = slm._state = slm._make_state(X, y)
        try:
            assert isinstance(st, bs.CatFitState) and st.dtype == "f64" and type(st.fm).__name__ == "FeatureMatrix64"
            assert [type(c).__name__ for c in st.children] == ["_ResidentFastFood64", "_ResidentLinear", "_ResidentRFF"]
            assert st.children[0].dX.dtype == np.float64
            if chunk:
                st.chunk = chunk   # four row chunks (the constructor keeps at least 256 rows a chunk)
                assert len(list(st._chunks())) == 4
            _check_elbo(slm, X, y, var, regs, [ls0, ls2], o, np.asarray(o["dhyp"]), "cat d=%d %s chunks=%s" % (d, "ard" if ard else "iso", 4 if chunk else 1))
        finally:
            st.release()


def test_elbo_of_a_lone_float64_fastfood_rbf_at_300_columns(monkeypatch):
    bs, Parameter, Positive, Bound, SLM = _slm_imports()
    rs = np.random.RandomState(11)
    N, d = 64, 300
    X = rs.randn(N, d)
    y = np.sin(X[:, :5] @ rs.randn(5)) + 0.1 * rs.randn(N)
    ff = bs.FastFoodRBF(nbases=512, Xdim=d, random_state=3, lenscale=Parameter(np.ones(d), Positive()), dtype="f64")
    assert (ff.d2, ff.k) == (512, 1)
    ls = np.linspace(3.0, 4.0, d)
    mats = (ff.B, ff.G, ff.PI, ff.S)
    Phi = orc.fastfood_transform(X, *mats, ls)
    o = orc.slm_elbo(Phi, y, 0.3, np.full(Phi.shape[1], 1.5), [slice(0, Phi.shape[1])], _slices3(orc.fastfood_grad(X, *mats, ls)))
    _no_host_features(monkeypatch, bs)
    slm = SLM(ff, resident_bases="all")
    slm.obj_ = -np.inf
    st = slm._state = slm._make_state(X, y)
    try:
        assert isinstance(st, bs.CatFitState) and st.dtype == "f64" and type(st.children[0]).__name__ == "_ResidentFastFood64"
        _check_elbo(slm, X, y, 0.3, 1.5, ls, o, np.asarray(o["dhyp"]), "lone FastFoodRBF d=300")
    finally:
        st.release()


def test_elbo_of_a_lone_float64_fastfood_gm_at_300_columns(monkeypatch):
    bs, Parameter, Positive, Bound, SLM = _slm_imports()
    rs = np.random.RandomState(12)
    N, d = 64, 300
    X = rs.randn(N, d)
    y = np.sin(X[:, :5] @ rs.randn(5)) + 0.1 * rs.randn(N)
    gm = bs.FastFoodGM(nbases=512, Xdim=d, random_state=5, mean=Parameter(np.zeros(d), Bound()),
                       lenscale=Parameter(np.ones(d), Positive()), dtype="f64", wide_chain=True)
    mean, ls = 0.02 * rs.randn(d), np.linspace(3.0, 4.0, d)
    mats = (gm.B, gm.G, gm.PI, gm.S)
    Phi = orc.fastfood_gm_transform(X, *mats, mean, ls)
    dM, dL = orc.fastfood_gm_grad(X, *mats, mean, ls)
    o = orc.slm_elbo(Phi, y, 0.3, np.full(Phi.shape[1], 1.5), [slice(0, Phi.shape[1])], _slices3(dM) + _slices3(dL))
    del dM, dL
    assert SLM(gm)._make_state(X, y) is None      # the default keyword: no resident float64 fit, as on the parent
    _no_host_features(monkeypatch, bs)
    slm = SLM(gm, resident_bases="all")
    slm.obj_ = -np.inf
    st = slm._state = slm._make_state(X, y)
    try:
        assert isinstance(st, bs.CatFitState) and st.dtype == "f64" and type(st.children[0]).__name__ == "_ResidentFastFoodGM64"
        _check_elbo(slm, X, y, 0.3, 1.5, [mean, ls], o, np.asarray(o["dhyp"]), "lone FastFoodGM d=300")
    finally:
        st.release()


def test_the_default_keyword_reports_the_parents_states():
    bs, Parameter, Positive, Bound, SLM = _slm_imports()
    rs = np.random.RandomState(0)
    X, y = rs.randn(50, 20), rs.randn(50)
    ff = bs.FastFoodRBF(nbases=64, Xdim=20, random_state=1, dtype="f64")
    st = SLM(ff)._make_state(X, y)
    assert type(st) is bs.DeviceFitState                          # the dense equivalent on the random Fourier kernels
    st.release()
    st = SLM(ff, resident_bases="fourier")._make_state(X, y)
    assert type(st) is bs.DeviceFitState
    st.release()
    f32 = bs.FastFoodRBF(nbases=64, Xdim=20, random_state=1)
    for kw in ({}, {"resident_bases": "all"}):                    # an f32 basis keeps its f32 chain state under either keyword
        st = SLM(f32, **kw)._make_state(X, y)
        assert type(st) is bs.CatFitState and st.dtype == "f32" and type(st.children[0]) is bs._ResidentFastFood
        st.release()
    gm = bs.FastFoodGM(nbases=64, Xdim=20, random_state=1, dtype="f64")
    assert SLM(gm)._make_state(X, y) is None
    assert (ff + bs.LinearBasis()).device_fit_state(X, y) is None


# ---- 4: the GLM step ---------------------------------------------------------------------------------------------------------------
def _glm_concat():
    """The ragged concatenation of tests/test_gpu_glm_f64.py (333 rows, K L = 28) with an f32 FastFoodRBF child (evaluated in
    float64 by the matrix) and a float64 FastFoodGM child on 12 columns (d2 = 16) in place of its generic child."""
    bs, lk, Parameter, Positive, GLM = g64._imports()
    d = 12
    rs = np.random.RandomState(3)
    X = rs.randn(gc.CONCAT["M"], d)
    five = list(range(5))
    b0 = bs.RandomMatern32(nbases=40, Xdim=5, random_state=1, lenscale=Parameter(np.ones(5), Positive()), apply_ind=five)
    b1 = bs.LinearBasis(onescol=True, apply_ind=five)
    b2 = bs.FastFoodRBF(nbases=24, Xdim=5, random_state=6, lenscale=Parameter(np.ones(5), Positive()), apply_ind=five)
    b3 = bs.FastFoodGM(nbases=16, Xdim=d, random_state=2, dtype="f64")
    ls0, ls2, mu, lsg = np.linspace(0.8, 1.3, 5), np.linspace(1.1, 0.7, 5), 0.1 * rs.randn(d), np.linspace(0.9, 1.6, d)
    X5 = X[:, :5]
    blocks = [orc.rff_transform(X5, b0.W, ls0), orc.linear_transform(X5, True), orc.fastfood_transform(X5, b2.B, b2.G, b2.PI, b2.S, ls2),
              orc.fastfood_gm_transform(X, b3.B, b3.G, b3.PI, b3.S, mu, lsg)]
    dM, dLs = orc.fastfood_gm_grad(X, b3.B, b3.G, b3.PI, b3.S, mu, lsg)
    grads = [_slices3(orc.rff_grad(X5, b0.W, ls0)), [], _slices3(orc.fastfood_grad(X5, b2.B, b2.G, b2.PI, b2.S, ls2)),
             _slices3(dM) + _slices3(dLs)]
    Phi = np.hstack(blocks)
    return X, b0 + b1 + b2 + b3, [ls0, ls2, mu, lsg], [1.2, 0.8, 1.5, 0.6], Phi, g64._pad_slabs(Phi, blocks, grads)


KINDS = ["_ResidentRFF", "_ResidentLinear", "_ResidentFastFood64", "_ResidentFastFoodGM64"]


def test_glm_step_with_fastfood_children_vs_oracle(monkeypatch):
    bs, lk, Parameter, Positive, GLM = g64._imports()
    K, L = gc.CONCAT["K"], gc.CONCAT["L"]
    X, cat, hyp, regs, Phi, slabs = _glm_concat()
    rs = np.random.RandomState(5)
    y = rs.poisson(np.exp(0.5 * np.sin(X[:, 0]))).astype(float)
    D = Phi.shape[1]
    assert D == int(cat.get_dim(X))
    m = 0.2 * rs.randn(D, K)
    C = rs.gamma(2., 0.5, size=(D, K))
    Ld, slices = cat.regularizer_diagonal(X, *regs)
    e = np.random.RandomState(9).randn(K * L, D).reshape(K, L, D)
    want = orc.glm_elbo(m, C, Ld, slices, "poisson_exp", [], (), Phi, slabs, y, e, 6.0)
    _no_host_features(monkeypatch, bs)
    glm = GLM(likelihood=lk.Poisson(), basis=cat, K=K, nsamples=L, random_state=9, dtype="f64", resident_bases="all")
    glm.B_, glm.D_ = 6.0, D
    try:
        got = g64._step(glm, m, C, regs, [], hyp, X, y)
        kinds = [type(c).__name__ for c, _, _ in glm._features().children]
    finally:
        glm._release_features()
    assert kinds == KINDS
    assert isinstance(got[1][4], list) and len(got[1][4]) == 4
    g64._check_step(got, want, "concat with FastFood children")
    # the default keyword keeps the generic children
    glm = GLM(likelihood=lk.Poisson(), basis=cat, K=K, nsamples=L, random_state=9, dtype="f64")
    feats = glm._features()
    try:
        assert [type(feats._child(b, X)).__name__ for b in cat.bases[2:]] == ["NoneType", "NoneType"]
        assert feats.make_resident(X) is False
    finally:
        glm._release_features()


def test_glm_resident_gather_equals_host_rows_bit_for_bit():
    bs, lk, Parameter, Positive, GLM = g64._imports()
    K, L, M = gc.CONCAT["K"], gc.CONCAT["L"], gc.CONCAT["M"]
    _, cat, hyp, regs, _, _ = _glm_concat()
    rs = np.random.RandomState(21)
    N = 500
    X = rs.randn(N, 12)
    y = rs.poisson(np.exp(0.5 * np.sin(X[:, 0]))).astype(float)
    D = int(cat.get_dim(X))
    m = 0.2 * rs.randn(D, K)
    C = rs.gamma(2., 0.5, size=(D, K))
    idx = rs.permutation(N)[:M]

    def model():
        glm = GLM(likelihood=lk.Poisson(), basis=cat, K=K, nsamples=L, random_state=9, dtype="f64", resident_bases="all")
        glm.B_, glm.D_ = 6.0, D
        return glm
    for det in (False, True):
        with g64._Deterministic(det):
            host = model()
            try:
                a = g64._step(host, m, C, regs, [], hyp, X[idx], y[idx])
            finally:
                host._release_features()
            res = model()
            try:
                assert res._features().make_resident(X, "all") is True
                res._resident_fit = True
                b = g64._step(res, m, C, regs, [], hyp, X[idx], y[idx], idx)
                kinds = [type(c).__name__ for c, _, _ in res._features().children]
            finally:
                res._resident_fit = False
                res._release_features()
        assert kinds == KINDS
        assert g64._bytes(a, basis_grads=det) == g64._bytes(b, basis_grads=det)
        assert normwise(g64._flat(a[1][4]), g64._flat(b[1][4])) < 1e-13


def test_a_seeded_fit_with_a_fastfood_child_equals_the_oracles_fit():
    """20 Adam steps of GeneralizedLinearModel(dtype="f64", resident_bases="all") on LinearBasis + FastFoodRBF (ARD, random length
    scales) against oracle.glm_fit, which takes the chain's dense equivalent V = fastfood_VX(I_d) as a random Fourier child (the
    same features and the same gradient slabs), at the float64 step's 1e-8."""
    from scipy.stats import gamma
    bs, lk, Parameter, Positive, GLM = g64._imports()
    rs = np.random.RandomState(21)
    N, d, n = 300, 3, 8
    X = rs.randn(N, d)
    y = rs.poisson(np.exp(0.6 * np.sin(X[:, 0]) + 0.3 * X[:, 1])).astype(float)
    K, L, maxiter, seed, gseed, batch, nstarts = 3, 6, 20, 17, 5, 64, 2
    ff = bs.FastFoodRBF(nbases=n, Xdim=d, random_state=3, lenscale=Parameter(gamma(4., scale=0.25), Positive(), shape=(d,)), dtype="f64")
    basis = bs.LinearBasis(onescol=True) + ff
    V = orc.fastfood_VX(np.eye(d), ff.B, ff.G, ff.PI, ff.S)
    regs, lss = [], []
    for b in basis.bases:
        r = b.regularizer
        regs.append(orc.ParamSpec(dist=r.dist, value=None if r.dist is not None else r.value, positive=True, shape=r.shape))
    lss = [orc.ParamSpec(value=[]), orc.ParamSpec(dist=ff.params.dist, positive=True, upper=ff.params.bounds.upper, shape=ff.params.shape)]
    o = orc.glm_fit(X, y, "poisson_exp", [], [("linear", True), ("rff", V, d)], regs, [], lss, K, L, batch, maxiter, nstarts, seed, gseed,
                    sgd_batch_size=batch)
    glm = GLM(lk.Poisson("exp"), basis, K=K, nsamples=L, batch_size=batch, maxiter=maxiter, nstarts=nstarts, random_state=seed,
              dtype="f64", resident_bases="all")
    np.random.seed(gseed)
    glm.fit(X, y)
    errs = {"m": normwise(glm.weights_, o[0]), "C": normwise(glm.covariance_, o[1]), "reg": normwise(g64._flat(glm.regularizer_), g64._flat(o[2])),
            "ls": normwise(g64._flat(glm.basis_hypers_), g64._flat(o[4]))}
    print("float64 fit with a FastFood child: %s" % {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) < gc.TOL_FIT, errs
    assert glm.random_.randn() == o[7]
