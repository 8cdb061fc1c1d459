"""FastFoodRBF on inputs wider than 256 columns: the wide chain kernel (rr_fastfood64_kernel, d2 = 512 .. 4096; handles from
rr_fastfood_create_wide) against exact references, and the basis class on top of it against the recorded reference.

Cases, data and checks live in tests/fastfood_wide_cases.py (the CPU half: tests/test_fastfood_wide_host.py).  VX is compared
bit for bit (d2 = 1024, 4096) or to one ulp (512, 2048), features are taken at exactly known phases within PHI_F32_BOUND /
PHI_F64_BOUND, device-resident calls write into sentinel-filled buffers, real-valued data is held element by element to the
forward error bound of the chain."""
import numpy as np
import pytest

import revrand_oracle as orc
from conftest import normwise

import fastfood_wide_cases as wc
from test_gpu_fastfood_exact import INV2PI, NP, PHI_F32_BOUND, PHI_F64_BOUND, TWO_PI_L, U, _chain_ld

pytestmark = pytest.mark.gpu

GOLDEN_SHAPES = [(300, 600, 4), (1000, 1500, 3), (2049, 4097, 2), (4096, 4096, 2)]


# ---- the chain kernel ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", wc.GRID, ids=wc.ids(wc.GRID))
def test_every_instance_is_exact(c):
    wc.run_and_check(c)


@pytest.mark.parametrize("c", wc.VARIANTS, ids=wc.ids(wc.VARIANTS))
def test_variants_and_untouched_elements(c):
    """Leading dimensions and pointer offsets that flip VEC on their own, through the device-resident call into a
    sentinel-filled buffer: the block is exact, every element around it untouched."""
    wc.run_and_check(c)


@pytest.mark.parametrize("c", wc.DTYPES, ids=wc.ids(wc.DTYPES))
def test_every_dtype_combination_is_exact(c):
    wc.run_and_check(c)


@pytest.mark.parametrize("c", wc.RP_CASES, ids=wc.ids(wc.RP_CASES))
def test_rows_per_workgroup_seam(c, monkeypatch):
    """RR_FF_ROWS_PER_BLOCK = 9 with ten rows: one workgroup whose waves take several rows each, and one more row."""
    monkeypatch.setenv("RR_FF_ROWS_PER_BLOCK", str(wc.RP))
    D, _ = wc.run_and_check(c)
    assert len({r.tobytes() for r in D.I}) == c.N  # (the rows really differ)


def test_host_call_across_a_chunk_seam():
    wc.run_and_check_seam()


@pytest.mark.parametrize("compute,d2,col0", wc.FEATMAT, ids=["%s-d2=%d-col0=%d" % f for f in wc.FEATMAT])
def test_feature_matrix_block_and_untouched_columns(compute, d2, col0):
    wc.run_featmat(compute, d2, col0)


# real-valued data: (N, d, nbases), one shape per d2 (the long double reference is a dense (d2, d2) product per block)
REAL_SHAPES = [(5, 300, 1024), (4, 1000, 1024), (3, 1500, 2048), (2, 4096, 4096)]


@pytest.mark.parametrize("compute", ["f32", "f64"])
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_real_valued_data_element_by_element(shape, compute):
    """As tests/test_gpu_fastfood_exact.py::test_real_valued_data_element_by_element: Gaussian x, the matrices of
    oracle.fastfood_matrices, ARD length scales, the reference the chain in long double over the tables as the library forms
    them.  Every element of VX within ((1 + u)^(2 log2 d2 + 4) - 1) A, A the chain over absolute values; Phi within 2 pi times
    that bound on the phase in revolutions plus the sine / cosine bound at an exact phase."""
    from revrand_amd import _hip
    N, d, nb = shape
    T = NP[compute]
    u = U[compute]
    rs = np.random.RandomState(N + d)
    X = rs.randn(N, d).astype(T)
    ls = np.linspace(0.6, 1.7, d)
    B, G, PI, S = orc.fastfood_matrices(nb, d, 5)
    k, d2 = B.shape
    ff = _hip.FastFoodHandle(d, d2, k, B, G, PI, S, compute=compute, wide=True)
    L = (1.0 / ls).astype(T)
    norm = float(d2) ** -1.5
    gamma = float(np.expm1((2 * int(np.log2(d2)) + 4) * np.log1p(u))) + 2.0 ** -59
    # (one long double chain up to the last diagonal serves both tables: a product with S in long double is one rounding of
    # 2^-64, granted below)
    V1, A1 = _chain_ld(X, L, B, G.astype(T), PI, np.ones_like(S))
    Srad, Srev = (S * norm).astype(T).astype(np.longdouble).ravel(), ((S * norm) * INV2PI).astype(T).astype(np.longdouble).ravel()
    V, A = V1 * Srad, A1 * np.abs(Srad)
    got = ff.vx(X, ls, out_dtype=T)
    err = np.abs(got.astype(np.longdouble) - V)
    ratio = float((err / (gamma * A + np.finfo(np.longdouble).tiny)).max())
    print("VX  %s %s: max error / bound %.3f" % (shape, compute, ratio))
    assert np.all(err <= gamma * A), ratio
    Vr, Ar = V1 * Srev, A1 * np.abs(Srev)
    f = Vr - np.rint(Vr)
    want = np.concatenate((np.cos(TWO_PI_L * f), np.sin(TWO_PI_L * f)), axis=1)
    got = ff.transform(X, ls, out_dtype=T)
    err = np.abs(got.astype(np.longdouble) * np.sqrt(np.longdouble(d2 * k)) - want)
    trig = PHI_F32_BOUND if compute == "f32" else PHI_F64_BOUND
    bound = np.tile(2 * np.pi * gamma * Ar + trig, (1, 2))
    ratio = float((err / bound).max())
    print("Phi %s %s: max error / bound %.3f, max |error| %.3e" % (shape, compute, ratio, float(err.max())))
    assert np.all(err <= bound), ratio


# ---- FastFoodRBF against the recorded reference -------------------------------------------------------------------------
def _basis(d, nb, ard, dtype="f32"):
    import revrand_amd.basis_functions as bs
    from revrand_amd.btypes import Parameter, Positive
    if ard:
        return bs.FastFoodRBF(nbases=nb, Xdim=d, random_state=3, dtype=dtype, lenscale=Parameter(np.ones(d), Positive()))
    return bs.FastFoodRBF(nbases=nb, Xdim=d, random_state=3, dtype=dtype)


def _phase_bound(b, X, ls, u):
    """Bound on the error of the phase in REVOLUTIONS of the chain in arithmetic u against the exact value, per row and column:
    ((1 + u)^m - 1) A with A the chain over absolute values -- |H| is all ones, so A[r, j d2 + e] = sum_i |x_ri / l_i| sum |G_j|
    |S_je| d2^-1.5 / 2 pi -- and m = 2 log2 d2 + 7 roundings: the 2 log2 d2 + 4 of the kernel's arithmetic (x / l, the
    butterflies, the product with G, the product with S, one for pow()) and the three table conversions 1 / l, G and
    S d2^-1.5 / 2 pi to the compute type, which the recorded float64 reference does not share."""
    m = 2 * int(np.log2(b.d2)) + 7
    gamma = float(np.expm1(m * np.log1p(u)))
    sx = (np.abs(X) / np.broadcast_to(np.asarray(ls, dtype=float), (X.shape[1],))).sum(axis=1)
    A = sx[:, None] * (np.abs(b.G).sum(axis=1)[:, None] * np.abs(b.S) * float(b.d2) ** -1.5 * INV2PI).ravel()[None, :]
    return gamma * A


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", GOLDEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transform_against_the_recorded_reference(shape, dtype, golden):
    """FastFoodRBF.transform at Xdim = 300, 1000, 2049, 4096, isotropic and ARD, against the reference's output at the stored
    columns.  Element by element: |Phi sqrt(n) - ref sqrt(n)| <= 2 pi (phase bound of this arithmetic + phase bound of the
    float64 reference) + the sine / cosine bound of the arithmetic at an exact phase + 1e-15 for the reference's own."""
    d, nb, N = shape
    g = golden("fastfood_wide")
    tag = "d%d" % d
    X, cols = g["X_" + tag].astype(np.float64), g["cols_" + tag]
    for name, ls, ard in (("iso", float(g["ls_iso"]), False), ("ard", g["ls_ard_" + tag], True)):
        b = _basis(d, nb, ard, dtype)
        P = b.transform(X, ls)
        assert P.shape == (N, 2 * b.n) and P.dtype == np.float64
        ph = _phase_bound(b, X, ls, U[dtype]) + _phase_bound(b, X, ls, U["f64"])
        bound = np.tile(2 * np.pi * ph + (PHI_F32_BOUND if dtype == "f32" else PHI_F64_BOUND) + 1e-15, (1, 2))[:, cols]
        err = np.abs(P[:, cols] - g["Phi_%s_%s" % (name, tag)]) * np.sqrt(b.n)
        print("%s %s %s: max |error| %.3e, max error / bound %.3f, smallest bound %.3e" % (tag, dtype, name, err.max(), (err / bound).max(), bound.min()))
        assert np.all(err <= bound), (name, float((err / bound).max()))
        if dtype == "f32":
            assert normwise(P[:, cols], g["Phi_%s_%s" % (name, tag)]) < 1e-3  # (what the narrow tests ask of a float32 basis)


@pytest.mark.parametrize("shape", GOLDEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grad_and_gram_against_the_recorded_reference(shape, golden):
    """grad (the dense equivalent of the chain on the random Fourier kernels' wide-input route) against the recorded reference,
    gram against P^T P and P^T y, at the tolerances of tests/test_gpu_large_xdim.py::test_fastfood_dense_equivalent_for_wide_inputs
    (1e-3 and 1e-4 normwise, float32 arithmetic)."""
    d, nb, N = shape
    g = golden("fastfood_wide")
    tag = "d%d" % d
    X, cols = g["X_" + tag].astype(np.float64), g["cols_" + tag]
    b = _basis(d, nb, False)
    dP = b.grad(X, float(g["ls_iso"]))
    assert dP.shape == (N, 2 * b.n)
    assert normwise(dP[:, cols], g["dPhi_iso_" + tag]) < 1e-3
    if d == 300:
        ba = _basis(d, nb, True)
        dA = ba.grad(X, g["ls_ard_" + tag])
        assert dA.shape == (N, 2 * ba.n, d)
        assert normwise(dA[:, g["gcols_" + tag], :], g["dPhi_ard_" + tag]) < 1e-3
    if d <= 1000:  # (the Gram of 8192 features and more is no part of this feature; two sizes show the route)
        y = np.sin(X[:, 0]) + 0.1 * np.arange(N)
        P = b.transform(X, 1.3)
        G, bv, _ = b.gram(X, y, 1.3)
        assert normwise(G, P.T @ P) < 1e-4 and normwise(bv, P.T @ y) < 1e-4
        # the same through the device group (one member here: the sharded route, the rows on device 0)
        Gd, bd, td = b.gram(X, y, 1.3, devices=[0])
        assert normwise(Gd, P.T @ P) < 1e-4 and normwise(bd, P.T @ y) < 1e-4 and abs(td - y @ y) < 1e-6 * (y @ y)


# ---- estimators at Xdim = 300 -------------------------------------------------------------------------------------------
def _oracle_ff_elbo(f, X, y, var, reg, ls):
    X64, y64 = X.astype(np.float64), y.astype(np.float64)
    Phi = orc.fastfood_transform(X64, f.B, f.G, f.PI, f.S, ls)
    dP = orc.fastfood_grad(X64, f.B, f.G, f.PI, f.S, ls)
    slabs = [dP] if dP.ndim == 2 else [dP[:, :, i] for i in range(dP.shape[2])]
    return orc.slm_elbo(Phi, y64, var, np.full(Phi.shape[1], reg), slice(None), slabs)


def test_resident_elbo_runs_the_chain_and_matches_the_oracle(monkeypatch):
    """StandardLinearModel._elbo on FastFoodRBF(Xdim = 300) with (X, y) resident, as
    tests/test_gpu_fastfood.py::test_fastfood_resident_elbo_runs_the_chain_and_matches_the_oracle at Xdim = 200: the chain route
    (a CatFitState over _ResidentFastFood) and the dense-equivalent route against the oracle, same tolerances."""
    import revrand_amd.basis_functions as bs
    from revrand_amd.slm import StandardLinearModel
    N, d, nb = 600, 300, 512
    rs = np.random.RandomState(N + d)
    X = rs.randn(N, d).astype(np.float32)
    y = (np.sin(X @ rs.randn(d) / np.sqrt(d)) + 0.1 * rs.randn(N)).astype(np.float32)
    f = bs.FastFoodRBF(nbases=nb, Xdim=d, random_state=3)
    ls, var, reg = 1.2, 0.3, 1.5
    out = {}
    for route in ("chain", "dense"):
        monkeypatch.setenv("RR_FASTFOOD_FIT", route)
        slm = StandardLinearModel(f)
        slm.obj_ = -np.inf
        slm._state = slm._make_state(X, y)
        assert type(slm._state).__name__ == ("CatFitState" if route == "chain" else "DeviceFitState")
        try:
            nelbo, (ndvar, ndreg, ndhyp) = slm._elbo(X, y, var, reg, ls)
            C = slm._state.best_covariance() if getattr(slm._state, "best_on_device", False) else slm.covariance_
        finally:
            slm._state.release()
            slm._state = None
        out[route] = (nelbo, ndvar, ndreg, np.atleast_1d(ndhyp), slm.weights_.copy(), np.array(C))
    ref = _oracle_ff_elbo(f, X, y, var, reg, ls)
    for route, (nelbo, ndvar, ndreg, ndhyp, m, C) in out.items():
        assert abs(-nelbo - ref["elbo"]) < 1e-4 * abs(ref["elbo"]), route
        assert abs(-ndvar - ref["dvar"]) < 1e-3 * abs(ref["dvar"]) and abs(-ndreg - ref["dreg"][0]) < 1e-3 * abs(ref["dreg"][0])
        assert normwise(-ndhyp, np.array(ref["dhyp"])) < 2e-3, route
        assert normwise(m, ref["m"]) < 1e-3 and normwise(C, ref["C"]) < 1e-3
    assert normwise(out["chain"][3], out["dense"][3]) < 2e-3


def test_slm_fit_and_predict_at_xdim_300():
    """StandardLinearModel.fit / predict on FastFoodRBF(Xdim = 300): a short fit ends with finite hyper-parameters and its
    predictive mean is the oracle's features at the learnt length scale times the learnt weights."""
    import revrand_amd.basis_functions as bs
    from revrand_amd.slm import StandardLinearModel
    rs = np.random.RandomState(5)
    X = rs.randn(400, 300).astype(np.float32)
    y = (np.sin(X @ rs.randn(300) / np.sqrt(300)) + 0.05 * rs.randn(400)).astype(np.float32)
    f = bs.FastFoodRBF(nbases=512, Xdim=300, random_state=1)
    slm = StandardLinearModel(f, maxiter=5).fit(X, y)
    Ey = slm.predict(X[:50])
    assert Ey.shape == (50,) and np.all(np.isfinite(Ey)) and np.isfinite(slm.var_)
    Phi = orc.fastfood_transform(X[:50].astype(np.float64), f.B, f.G, f.PI, f.S, float(np.ravel(slm.hypers_)[0]))
    assert normwise(Ey, Phi @ slm.weights_) < 1e-3


def test_glm_minibatch_step_vs_oracle():
    """One SVI step (GeneralizedLinearModel._elbo) on FastFoodRBF(Xdim = 300) + a bias column against oracle.glm_elbo, modelled
    on tests/test_gpu_large_xdim.py::test_glm_minibatch_step_vs_oracle: objective, dm, dC and the length-scale gradient."""
    import revrand_amd.basis_functions as bs
    import revrand_amd.likelihoods as lk
    from revrand_amd import GeneralizedLinearModel as GLM
    rs = np.random.RandomState(3)
    M, d, K, L = 333, 300, 3, 5
    X = rs.randn(M, d) / np.sqrt(d / 8.0)
    y = rs.poisson(np.exp(0.5 * np.sin(X[:, 0] * 3))).astype(float)
    f = bs.FastFoodRBF(nbases=512, Xdim=d, random_state=1)
    cat = f + bs.LinearBasis(onescol=True)
    hyp = [1.1]
    Phi = np.hstack((orc.fastfood_transform(X, f.B, f.G, f.PI, f.S, 1.1), orc.linear_transform(X, True)))
    dP = orc.fastfood_grad(X, f.B, f.G, f.PI, f.S, 1.1)
    dPs = [np.hstack((dP, np.zeros((M, d + 1))))]
    D = Phi.shape[1]
    m = 0.2 * rs.randn(D, K)
    C = rs.gamma(2., 0.5, size=(D, K))
    regs = [1.2, 0.8]
    Ld, slices = cat.regularizer_diagonal(X, *regs)
    e = np.stack([np.random.RandomState(9).randn(K * L, D)[k * L:(k + 1) * L] for k in range(K)])
    want = orc.glm_elbo(m, C, Ld, slices, "poisson_exp", [], (), Phi, dPs, y, e, 6.0)
    glm = GLM(likelihood=lk.Poisson(), basis=cat, K=K, nsamples=L, random_state=9)
    glm.B_, glm.D_ = 6.0, D
    glm._GeneralizedLinearModel__it = -1
    nobj, (ndm, ndC, dL, dlp, dbp) = glm._elbo(m.copy(), C.copy(), regs, [], hyp, X, y)
    glm._release_features()
    assert abs(nobj - want[0]) < 2e-4 * abs(want[0])
    assert normwise(ndm, want[1][0]) < 1e-3 and normwise(ndC, want[1][1]) < 1e-3
    flat = np.ravel(dbp).astype(float)  # (one isotropic length scale: a scalar, or a list holding it)
    assert flat.shape == (1,)
    assert normwise(flat, np.array(want[1][4])) < 2e-3


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_range_of_the_wide_entry_point():
    """FastFoodRBF(Xdim = 5000) is refused naming 4096; so is a d2 = 8192 handle by rr_fastfood_create_wide; d2 = 256 there
    points at rr_fastfood_create."""
    import ctypes
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    with pytest.raises(ValueError, match="4096"):
        bs.FastFoodRBF(nbases=8, Xdim=5000, random_state=0)
    rs = np.random.RandomState(0)
    B, G = rs.randint(2, size=(1, 8192)) * 2 - 1, rs.randn(1, 8192)
    PI, S = rs.permutation(8192)[None, :], np.ones((1, 8192))
    with pytest.raises(_hip.HipError, match="4096"):
        _hip.FastFoodHandle(5000, 8192, 1, B, G, PI, S, wide=True)
    dev = _hip.get_device()
    a = [np.ascontiguousarray(B[:, :256], dtype=np.int64), np.ascontiguousarray(G[:, :256]), np.arange(256, dtype=np.int64)[None, :],
         np.ones((1, 256))]
    h = ctypes.c_void_p()
    with pytest.raises(_hip.HipError, match="served by rr_fastfood_create"):
        _hip._check(dev.lib, dev.lib.rr_fastfood_create_wide(dev.ctx, _hip.RR_F32, 200, 256, 1,
                                                             *[x.ctypes.data_as(ctypes.c_void_p) for x in a], ctypes.byref(h)))
    assert not h.value
    # a handle class that does not ask for the wide entry keeps the narrow one's refusal
    with pytest.raises(_hip.HipError, match="256"):
        _hip.FastFoodHandle(300, 512, 1, B[:, :512], G[:, :512], np.arange(512)[None, :], S[:, :512])


def test_mixture_mode_refuses_a_wide_handle():
    """The GM entry points on a wide handle: RR_ERR_UNSUPPORTED, the message the narrow handles give beyond d2 = 256."""
    from revrand_amd import _hip
    c = wc.GRID[0]
    ff = wc.handle(c, wc.case_data(c))
    with pytest.raises(_hip.HipError, match="256"):
        ff.gm_transform(np.zeros((2, c.d)), np.zeros(c.d), np.ones(c.d))


def test_fastfood_gm_keeps_its_range():
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    with pytest.raises(_hip.HipError, match="256"):
        bs.FastFoodGM(nbases=8, Xdim=300).transform(np.zeros((2, 300)))
