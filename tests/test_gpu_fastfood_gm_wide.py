"""FastFoodGM on inputs wider than 256 columns behind ``wide_chain=True``: the mixture mode of the wide chain kernel
(rr_fastfood64_kernel<..., GM>, d2 = 512 .. 4096; handles from rr_fastfood_create_wide_gm) against exact references, and the
basis class on top of it against the recorded reference and the oracle's estimators.

Cases, data and checks live in tests/fastfood_gm_wide_cases.py (the CPU half: tests/test_fastfood_gm_wide_host.py).  Features
are taken at exactly known phases (I +- M) / 16 revolutions within PHI_F32_BOUND / PHI_F64_BOUND, device-resident calls write
into sentinel-filled buffers, real-valued data is held element by element to the forward error bound of the chain plus that
of the mean shift's reduction."""
import ctypes

import numpy as np
import pytest

import revrand_oracle as orc
from conftest import normwise

import fastfood_gm_wide_cases as gc
import fastfood_wide_cases as wc
from test_gpu_fastfood_exact import INV2PI, NP, PHI_F32_BOUND, PHI_F64_BOUND, TWO_PI_L, U, _chain_ld, _exact_cos_sin
from test_gpu_fastfood_wide import _phase_bound

pytestmark = pytest.mark.gpu

GOLDEN_SHAPES = [(300, 600, 4), (1000, 1500, 3), (2049, 4097, 2), (4096, 4096, 2)]


# ---- the chain kernel's mixture mode ------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", gc.GRID, ids=gc.ids(gc.GRID))
def test_every_instance_is_exact(c):
    gc.run_and_check(c)


@pytest.mark.parametrize("c", gc.VARIANTS, ids=gc.ids(gc.VARIANTS))
def test_variants_and_untouched_elements(c):
    """Leading dimensions and pointer offsets that flip VEC on their own, through the device-resident call into a
    sentinel-filled buffer: the block is exact, every element around it untouched."""
    gc.run_and_check(c)


@pytest.mark.parametrize("c", gc.DTYPES, ids=gc.ids(gc.DTYPES))
def test_every_dtype_combination_is_exact(c):
    gc.run_and_check(c)


@pytest.mark.parametrize("c", gc.RP_CASES, ids=gc.ids(gc.RP_CASES))
def test_rows_per_workgroup_seam(c, monkeypatch):
    """RR_FF_ROWS_PER_BLOCK = 9 with ten rows: one workgroup whose waves take several rows each, and one more row -- the x
    fetched a row ahead and its mX stay paired (every row has its own I and, but for chance, its own M)."""
    monkeypatch.setenv("RR_FF_ROWS_PER_BLOCK", str(gc.RP))
    D, _ = gc.run_and_check(c)
    assert len({r.tobytes() for r in D.I}) == c.N and len(set(D.M.tolist())) >= c.N - 2


@pytest.mark.parametrize("c", gc.ZERO_MEAN_CASES, ids=gc.ids(gc.ZERO_MEAN_CASES))
def test_zero_mean_gives_two_identical_halves(c):
    D = gc.case_data(c)
    D.m, D.M, D.mean = np.zeros(c.d, dtype=np.int64), np.zeros(c.N, dtype=np.int64), np.zeros(c.d)
    got = gc.run_case(c, D)
    n = c.d2 * c.k
    assert np.array_equal(got[:, :2 * n].view(np.uint8), got[:, 2 * n:].view(np.uint8))
    gc.check_phi(c, D, got)


def test_mean_shift_survives_a_length_scale_beyond_the_float32_range():
    """lenscale = 1e60 on every dimension that carries a non-zero: 1 / l rounds to zero in float32, the chain's phase is zero,
    and the features are exact cos / sin of +- M / 16 revolutions -- mX is taken on the raw x, not on x / l."""
    c = gc.HUGE_LS_CASE
    D = gc.case_data(c)
    ls = np.where((D.X != 0).any(axis=0), 1e60, D.ls)
    assert np.all(np.float32(1.0 / ls[(D.X != 0).any(axis=0)]) == 0) and np.abs(D.M).min() >= 0 and np.abs(D.M).max() > 16
    got = gc.run_case(c, D, ls=ls)
    n = c.d2 * c.k
    mx = np.broadcast_to((D.M.astype(np.float64) / 16)[:, None], (c.N, n))
    want = np.concatenate(_exact_cos_sin(mx) + _exact_cos_sin(-mx), axis=1)
    err = np.abs(got.astype(np.longdouble) * np.sqrt(np.longdouble(2 * n)) - want).astype(np.float64)
    print("lenscale = 1e60: max |error| %.3e (bound %.3e), max |mX| %.1f rev" % (err.max(), PHI_F32_BOUND, np.abs(mx).max()))
    assert np.all(err <= PHI_F32_BOUND)


@pytest.mark.parametrize("compute,d2,col0", gc.FEATMAT, ids=["%s-d2=%d-col0=%d" % f for f in gc.FEATMAT])
def test_feature_matrix_block_and_untouched_columns(compute, d2, col0):
    gc.run_featmat(compute, d2, col0)


# real-valued data: (N, d, nbases), one shape per d2 (the long double reference is a dense (d2, d2) product per block)
REAL_SHAPES = [(5, 300, 1024), (4, 1000, 1024), (3, 1500, 2048), (2, 4096, 4096)]


@pytest.mark.parametrize("compute", ["f32", "f64"])
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_real_valued_data_element_by_element(shape, compute):
    """As tests/test_gpu_fastfood_wide.py::test_real_valued_data_element_by_element, with the mean shift: Gaussian x and mean,
    the matrices of oracle.fastfood_matrices, ARD length scales.  The reference is the chain in long double (`_chain_ld`) over
    the tables as the library forms them, mX in long double over mrev = T(mean * inv2pi) as ff_prepare_mean forms it.  Per
    element
        |Phi sqrt(2n) - ref| <= 2 pi (gamma_chain A + gamma_m sum_i |x_i mrev_i| + u (|ph| + |mX|)) + trig
    with gamma_chain, A and trig exactly those of that test, the third term the rounding of ph +- mX, and
    gamma_m = (1 + u)^m - 1, m = (R + 6) + 1: the kernel comment's longest rounding path of the reduction (R FMAs per lane plus
    six butterfly levels, R = d2 / 64) plus one for the table conversion."""
    from revrand_amd import _hip
    N, d, nb = shape
    T = NP[compute]
    u = U[compute]
    rs = np.random.RandomState(N + d)
    X = rs.randn(N, d).astype(T)
    mean = 0.3 * rs.randn(d)
    ls = np.linspace(0.6, 1.7, d)
    B, G, PI, S = orc.fastfood_matrices(nb, d, 5)
    k, d2 = B.shape
    n = d2 * k
    ff = _hip.FastFoodHandle(d, d2, k, B, G, PI, S, compute=compute, wide="gm")
    L = (1.0 / ls).astype(T)
    norm = float(d2) ** -1.5
    gamma = float(np.expm1((2 * int(np.log2(d2)) + 4) * np.log1p(u))) + 2.0 ** -59
    gamma_m = float(np.expm1((d2 // 64 + 6 + 1) * np.log1p(u))) + 2.0 ** -59
    Srev = ((S * norm) * INV2PI).astype(T)
    Vr, Ar = _chain_ld(X, L, B, G.astype(T), PI, Srev)
    mrev = (mean * INV2PI).astype(T).astype(np.longdouble)
    terms = X.astype(np.longdouble) * mrev
    mX, aX = terms.sum(axis=1)[:, None], np.abs(terms).sum(axis=1)[:, None]
    assert float(np.abs(mX).max()) > 0.25  # (the shift is worth a good part of a revolution)
    blocks = []
    for t in (Vr + mX, Vr - mX):
        f = t - np.rint(t)
        blocks += [np.cos(TWO_PI_L * f), np.sin(TWO_PI_L * f)]
    want = np.concatenate(blocks, axis=1)
    got = ff.gm_transform(X, mean, ls, out_dtype=T)
    assert got.shape == (N, 4 * n)
    err = np.abs(got.astype(np.longdouble) * np.sqrt(np.longdouble(2 * n)) - want)
    trig = PHI_F32_BOUND if compute == "f32" else PHI_F64_BOUND
    bound = np.tile(2 * np.pi * (gamma * Ar + gamma_m * aX + u * (np.abs(Vr) + np.abs(mX))) + trig, (1, 4))
    ratio = float((err / bound).max())
    print("GM  %s %s: max error / bound %.3f, max |error| %.3e, max |mX| %.2f rev" % (shape, compute, ratio, float(err.max()),
                                                                                  float(np.abs(mX).max())))
    assert np.all(err <= bound), ratio


# ---- FastFoodGM(wide_chain=True) against the recorded reference -----------------------------------------------------------
def _gm(d, nb, dtype="f32", seed=3):
    import revrand_amd.basis_functions as bs
    from revrand_amd.btypes import Bound, Parameter, Positive
    return bs.FastFoodGM(nbases=nb, Xdim=d, random_state=seed, dtype=dtype, mean=Parameter(np.zeros(d), Bound()),
                         lenscale=Parameter(np.ones(d), Positive()), wide_chain=True)


def _dot_bound(X, mean, u, m):
    """Bound on the error of mX = x . mean / 2 pi in REVOLUTIONS summed with m roundings per path in arithmetic u."""
    return float(np.expm1(m * np.log1p(u))) * (np.abs(X) * np.abs(mean) * INV2PI).sum(axis=1)[:, None]


@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("shape", GOLDEN_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_transform_against_the_recorded_reference(shape, dtype, golden):
    """FastFoodGM(wide_chain=True).transform at Xdim = 300, 1000, 2049, 4096 against the reference's output at the stored
    columns, element by element:
        |Phi sqrt(2n) - ref sqrt(2n)| <= 2 pi (chain(u) + chain(u64) + dot(u) + dot(u64) + add(u)) + trig + 1e-15
    chain(.) = `_phase_bound` of tests/test_gpu_fastfood_wide.py for this arithmetic and for the reference's float64; dot(u) the
    reduction of mX with R + 6 roundings on its longest path plus the conversion of mean / 2 pi to the compute type and its
    product with 1 / 2 pi (R + 8); dot(u64) the reference's float64 dot product, at most d roundings on a path whatever its
    summation order; add(u) = u (A + sum |x_i mean_i| / 2 pi) >= u |ph +- mX|, the rounding of the sum the kernel forms, A the
    absolute-value chain inside `_phase_bound`; trig the sine / cosine bound of the arithmetic at an exact phase, 1e-15 for the
    reference's own.  float32 also: normwise < 1e-3, the project's float32 tolerance."""
    d, nb, N = shape
    g = golden("fastfood_gm_wide")
    tag = "d%d" % d
    X, cols, mean, ls = g["X_" + tag].astype(np.float64), g["cols_" + tag], g["mean_" + tag], g["ls_ard_" + tag]
    b = _gm(d, nb, dtype)
    P = b.transform(X, mean, ls)
    assert P.shape == (N, 4 * b.n) and P.dtype == np.float64
    u = U[dtype]
    chain = _phase_bound(b, X, ls, u)
    m_chain = 2 * int(np.log2(b.d2)) + 7
    A = chain / float(np.expm1(m_chain * np.log1p(u)))
    sxm = (np.abs(X) * np.abs(mean) * INV2PI).sum(axis=1)[:, None]
    ph = chain + _phase_bound(b, X, ls, U["f64"]) + _dot_bound(X, mean, u, b.d2 // 64 + 8) + _dot_bound(X, mean, U["f64"], d) \
        + u * (A + sxm)
    bound = np.tile(2 * np.pi * ph + (PHI_F32_BOUND if dtype == "f32" else PHI_F64_BOUND) + 1e-15, (1, 4))[:, cols]
    err = np.abs(P[:, cols] - g["Phi_" + tag]) * np.sqrt(2 * b.n)
    print("%s %s: max |error| %.3e, max error / bound %.3f, smallest bound %.3e" % (tag, dtype, err.max(), (err / bound).max(), bound.min()))
    assert np.all(err <= bound), float((err / bound).max())
    if dtype == "f32":
        assert normwise(P[:, cols], g["Phi_" + tag]) < 1e-3


# ---- estimators at Xdim = 300 -------------------------------------------------------------------------------------------
def _gm_slabs(b, X64, mean, ls, pad=0):
    """The 2 d slabs [dPhi/dmean_0 .. dPhi/dmean_{d-1}, dPhi/dl_0 .. dPhi/dl_{d-1}] of oracle.fastfood_gm_grad, one at a time
    (the two (N, 4n, d) tensors are 3 GB each at N = 600, n = 512, d = 300): the oracle's own expressions with the chain's
    linearity used once -- fastfood_VX(X e_i / l_i^2) = (x_i / l_i^2) fastfood_VX(I)[i] -- and held to orc.fastfood_gm_grad
    itself on the first rows by the caller.  `pad`: zero columns appended (the other children of a concatenation)."""
    V = orc.fastfood_VX(X64 / ls, b.B, b.G, b.PI, b.S)
    VI = orc.fastfood_VX(np.eye(b.d), b.B, b.G, b.PI, b.S)
    mX = (X64 @ mean)[:, None]
    msp, msm, cp, cm = -np.sin(V + mX), -np.sin(V - mX), np.cos(V + mX), np.cos(V - mX)
    rt = np.sqrt(2 * V.shape[1])
    z = np.zeros((X64.shape[0], pad))
    Tm = np.concatenate((msp, cp, -msm, -cm, z), axis=1) / rt   # (x_i times this: dPhi / dmean_i)
    Tl = np.concatenate((msp, cp, msm, cm, z), axis=1) / rt     # (dV_i, tiled over the four blocks, times this: dPhi / dl_i)
    for i in range(b.d):
        yield X64[:, i:i + 1] * Tm
    for i in range(b.d):
        yield (-(X64[:, i:i + 1] / ls[i] ** 2) * np.concatenate((np.tile(VI[i], 4), z[0]))[None, :]) * Tl


@pytest.fixture(scope="module")
def fit300():
    """One data set, basis and oracle evaluation shared by the estimator tests at Xdim = 300 (N = 600, nbases = 512: F = 2048)."""
    N, d, nb = 600, 300, 512
    rs = np.random.RandomState(N + d)
    X = rs.randn(N, d).astype(np.float32)
    y = (np.sin(X @ rs.randn(d) / np.sqrt(d)) + 0.1 * rs.randn(N)).astype(np.float32)
    b = _gm(d, nb)
    mean, ls = 0.3 * rs.randn(d) / np.sqrt(d / 8.0), np.linspace(0.8, 1.4, d)
    var, reg = 0.3, 1.5
    X64 = X.astype(np.float64)
    Phi = orc.fastfood_gm_transform(X64, b.B, b.G, b.PI, b.S, mean, ls)
    # the lazy slabs are the oracle's gradient: all 2 d of them on the first rows
    dM, dL = orc.fastfood_gm_grad(X64[:3], b.B, b.G, b.PI, b.S, mean, ls)
    head = list(_gm_slabs(b, X64[:3], mean, ls))
    assert normwise(np.stack(head[:d], axis=2), dM) < 1e-12 and normwise(np.stack(head[d:], axis=2), dL) < 1e-12
    ref = orc.slm_elbo(Phi, y.astype(np.float64), var, np.full(Phi.shape[1], reg), slice(None), _gm_slabs(b, X64, mean, ls))
    return dict(X=X, y=y, b=b, mean=mean, ls=ls, var=var, reg=reg, Phi=Phi, ref=ref)


def test_resident_elbo_runs_the_chain_and_matches_the_oracle(fit300):
    """StandardLinearModel._elbo on FastFoodGM(Xdim = 300, wide_chain=True) with (X, y) resident: a CatFitState over
    _ResidentFastFoodGM on the chain (dense is False), against orc.slm_elbo over orc.fastfood_gm_transform / fastfood_gm_grad at
    the tolerances of tests/test_gpu_fastfood_wide.py::test_resident_elbo_runs_the_chain_and_matches_the_oracle."""
    from revrand_amd.slm import StandardLinearModel
    f = fit300
    b, X, y, d = f["b"], f["X"], f["y"], 300
    slm = StandardLinearModel(b)
    slm.obj_ = -np.inf
    slm._state = slm._make_state(X, y)
    assert type(slm._state).__name__ == "CatFitState"
    child = slm._state.children[0]
    assert type(child).__name__ == "_ResidentFastFoodGM" and child.dense is False and child.ff.wide_gm
    try:
        nelbo, (ndvar, ndreg, ndhyp) = slm._elbo(X, y, f["var"], f["reg"], [f["mean"], f["ls"]])
        C = slm._state.best_covariance() if getattr(slm._state, "best_on_device", False) else slm.covariance_
    finally:
        slm._state.release()
        slm._state = None
    ref = f["ref"]
    assert isinstance(ndhyp, list) and len(ndhyp) == 2 and ndhyp[0].shape == ndhyp[1].shape == (d,)
    print("elbo %.6e (oracle %.6e); dmean %.2e, dlenscale %.2e normwise" % (-nelbo, ref["elbo"],
          normwise(-ndhyp[0], np.array(ref["dhyp"][:d])), normwise(-ndhyp[1], np.array(ref["dhyp"][d:]))))
    assert abs(-nelbo - ref["elbo"]) < 1e-4 * abs(ref["elbo"])
    assert abs(-ndvar - ref["dvar"]) < 1e-3 * abs(ref["dvar"]) and abs(-ndreg - ref["dreg"][0]) < 1e-3 * abs(ref["dreg"][0])
    assert normwise(-ndhyp[0], np.array(ref["dhyp"][:d])) < 2e-3      # d ELBO / d mean
    assert normwise(-ndhyp[1], np.array(ref["dhyp"][d:])) < 2e-3      # d ELBO / d lenscale
    assert normwise(slm.weights_, ref["m"]) < 1e-3 and normwise(C, ref["C"]) < 1e-3


def test_predict_moments_at_xdim_300(fit300):
    f = fit300
    ref = f["ref"]
    Ey, Vf = f["b"].predict_moments(f["X"][:50], [f["mean"], f["ls"]], ref["m"], ref["C"])
    Eo, Vo = orc.slm_predict_moments(f["Phi"][:50], ref["m"], ref["C"], 0.0)
    assert normwise(Ey, Eo) < 1e-3 and normwise(Vf, Vo) < 1e-3


@pytest.mark.parametrize("d,nb", [(300, 512), (1000, 1024)])
def test_gram_against_the_features(d, nb):
    """gram and gram(devices=[0]) against P^T P and P^T y of this basis' own transform (1e-4, as the wide FastFoodRBF test)."""
    N = 64
    rs = np.random.RandomState(d)
    X = rs.randn(N, d).astype(np.float32)
    y = np.sin(X[:, 0]) + 0.1 * np.arange(N)
    mean, ls = 0.3 * rs.randn(d) / np.sqrt(d / 8.0), np.linspace(0.8, 1.4, d)
    b = _gm(d, nb)
    P = b.transform(X, mean, ls)
    assert P.shape == (N, 4 * b.n)
    G, bv, _ = b.gram(X, y, mean, ls)
    assert normwise(G, P.T @ P) < 1e-4 and normwise(bv, P.T @ y) < 1e-4
    Gd, bd, td = b.gram(X, y, mean, ls, devices=[0])
    assert normwise(Gd, P.T @ P) < 1e-4 and normwise(bd, P.T @ y) < 1e-4 and abs(td - y @ y) < 1e-6 * (y @ y)


def test_slm_fit_and_predict_at_xdim_300():
    """A five-iteration StandardLinearModel.fit on FastFoodGM(Xdim = 300, wide_chain=True), alone and as a child of a
    concatenation: finite hyper-parameters, and the predictive mean is the oracle's features at the learnt parameters times the
    learnt weights."""
    import revrand_amd.basis_functions as bs
    from revrand_amd.slm import StandardLinearModel
    rs = np.random.RandomState(5)
    X = rs.randn(400, 300).astype(np.float32)
    y = (np.sin(X @ rs.randn(300) / np.sqrt(300)) + 0.05 * rs.randn(400)).astype(np.float32)
    X64 = X[:50].astype(np.float64)
    f = bs.FastFoodGM(nbases=512, Xdim=300, random_state=1, wide_chain=True)
    slm = StandardLinearModel(f, maxiter=5).fit(X, y)
    Ey = slm.predict(X[:50])
    assert Ey.shape == (50,) and np.all(np.isfinite(Ey)) and np.isfinite(slm.var_)
    mean, ls = (np.asarray(h, dtype=float) for h in slm.hypers_)
    assert mean.shape == ls.shape == (300,) and np.all(np.isfinite(mean)) and np.all(ls > 0)
    Phi = orc.fastfood_gm_transform(X64, f.B, f.G, f.PI, f.S, mean, ls)
    assert normwise(Ey, Phi @ slm.weights_) < 1e-3
    # as a child of a concatenation: the resident state takes every child
    f2 = bs.FastFoodGM(nbases=512, Xdim=300, random_state=2, wide_chain=True)
    cat = f2 + bs.LinearBasis(onescol=True)
    slm = StandardLinearModel(cat, maxiter=5)
    slm.obj_ = -np.inf
    state = slm._make_state(X, y)
    try:
        assert type(state).__name__ == "CatFitState" and [type(c).__name__ for c in state.children][0] == "_ResidentFastFoodGM"
    finally:
        state.release()
    slm = StandardLinearModel(cat, maxiter=5).fit(X, y)
    Ey = slm.predict(X[:50])
    mean, ls = (np.asarray(h, dtype=float) for h in slm.hypers_[:2])
    Phi = np.hstack((orc.fastfood_gm_transform(X64, f2.B, f2.G, f2.PI, f2.S, mean, ls), orc.linear_transform(X64, True)))
    assert normwise(Ey, Phi @ slm.weights_) < 1e-3


def test_glm_minibatch_step_vs_oracle():
    """One SVI step (GeneralizedLinearModel._elbo, the step-per-call host loop through MinibatchFeatures) on
    FastFoodGM(Xdim = 300, wide_chain=True) + a bias column against oracle.glm_elbo, at the tolerances of
    tests/test_gpu_fastfood_wide.py::test_glm_minibatch_step_vs_oracle: objective, dm, dC, and BOTH the mean and the
    length-scale gradient."""
    import revrand_amd.basis_functions as bs
    import revrand_amd.likelihoods as lk
    from revrand_amd import GeneralizedLinearModel as GLM
    rs = np.random.RandomState(3)
    M, d, K, L = 333, 300, 3, 5
    X = rs.randn(M, d) / np.sqrt(d / 8.0)
    y = rs.poisson(np.exp(0.5 * np.sin(X[:, 0] * 3))).astype(float)
    f = bs.FastFoodGM(nbases=512, Xdim=d, random_state=1, wide_chain=True)
    cat = f + bs.LinearBasis(onescol=True)
    mean, ls = 0.3 * rs.randn(d), np.linspace(0.8, 1.4, d)
    hyp = [mean, ls]
    Phi = np.hstack((orc.fastfood_gm_transform(X, f.B, f.G, f.PI, f.S, mean, ls), orc.linear_transform(X, True)))
    dM, dL = orc.fastfood_gm_grad(X[:3], f.B, f.G, f.PI, f.S, mean, ls)
    head = list(_gm_slabs(f, X[:3], mean, ls))
    assert normwise(np.stack(head[:d], axis=2), dM) < 1e-12 and normwise(np.stack(head[d:], axis=2), dL) < 1e-12
    D = Phi.shape[1]
    m = 0.2 * rs.randn(D, K)
    C = rs.gamma(2., 0.5, size=(D, K))
    regs = [1.2, 0.8]
    Ld, slices = cat.regularizer_diagonal(X, *regs)
    e = np.stack([np.random.RandomState(9).randn(K * L, D)[k * L:(k + 1) * L] for k in range(K)])
    want = orc.glm_elbo(m, C, Ld, slices, "poisson_exp", [], (), Phi, _gm_slabs(f, X, mean, ls, pad=d + 1), y, e, 6.0)
    glm = GLM(likelihood=lk.Poisson(), basis=cat, K=K, nsamples=L, random_state=9)
    glm.B_, glm.D_ = 6.0, D
    glm._GeneralizedLinearModel__it = -1
    nobj, (ndm, ndC, dLr, dlp, dbp) = glm._elbo(m.copy(), C.copy(), regs, [], hyp, X, y)
    glm._release_features()
    assert abs(nobj - want[0]) < 2e-4 * abs(want[0])
    assert normwise(ndm, want[1][0]) < 1e-3 and normwise(ndC, want[1][1]) < 1e-3
    assert isinstance(dbp, list) and [np.shape(v) for v in dbp] == [(d,), (d,)]
    wantb = np.array(want[1][4])
    print("GLM step: dmean %.2e, dlenscale %.2e normwise" % (normwise(dbp[0], wantb[:d]), normwise(dbp[1], wantb[d:])))
    assert normwise(np.asarray(dbp[0], dtype=float), wantb[:d]) < 2e-3     # d / d mean
    assert normwise(np.asarray(dbp[1], dtype=float), wantb[d:]) < 2e-3     # d / d lenscale


# ---- refusals ---------------------------------------------------------------------------------------------------------------
def test_range_of_the_wide_gm_entry_point():
    """rr_fastfood_create_wide_gm at d2 = 8192 names 4096; at d2 = 256 it points at rr_fastfood_create."""
    from revrand_amd import _hip
    rs = np.random.RandomState(0)
    B, G = rs.randint(2, size=(1, 8192)) * 2 - 1, rs.randn(1, 8192)
    PI, S = rs.permutation(8192)[None, :], np.ones((1, 8192))
    with pytest.raises(_hip.HipError, match="4096"):
        _hip.FastFoodHandle(5000, 8192, 1, B, G, PI, S, wide="gm")
    dev = _hip.get_device()
    a = [np.ascontiguousarray(B[:, :256], dtype=np.int64), np.ascontiguousarray(G[:, :256]), np.arange(256, dtype=np.int64)[None, :],
         np.ones((1, 256))]
    h = ctypes.c_void_p()
    with pytest.raises(_hip.HipError, match="served by rr_fastfood_create"):
        _hip._check(dev.lib, dev.lib.rr_fastfood_create_wide_gm(dev.ctx, _hip.RR_F32, 200, 256, 1,
                                                                *[x.ctypes.data_as(ctypes.c_void_p) for x in a], ctypes.byref(h)))
    assert not h.value
    # the class takes the narrow entry point at d2 <= 256 whatever the keyword: the mixture mode of the 16-lane kernels
    ff = _hip.FastFoodHandle(200, 256, 1, *a, wide="gm")
    assert ff.wide_gm is False and ff.gm_chain_ok


def test_materialised_grad_keeps_its_refusal():
    """FastFoodGM(wide_chain=True).grad at Xdim = 300: the dense route's message, as without the keyword at Xdim <= 256."""
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    b = bs.FastFoodGM(nbases=8, Xdim=300, random_state=0, wide_chain=True)
    with pytest.raises(_hip.HipError, match="gm: d=300 is not supported"):
        b.grad(np.zeros((2, 300)))


def test_a_plain_wide_handle_still_refuses_the_mixture_mode():
    """On this library too: a handle from rr_fastfood_create_wide refuses the GM entry points with the narrow handles' message,
    and FastFoodGM without the keyword refuses Xdim = 300."""
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    c = wc.GRID[0]
    ff = wc.handle(c, wc.case_data(c))
    assert ff.wide_gm is False and not ff.gm_chain_ok
    with pytest.raises(_hip.HipError, match="256"):
        ff.gm_transform(np.zeros((2, c.d)), np.zeros(c.d), np.ones(c.d))
    with pytest.raises(_hip.HipError, match="256"):
        bs.FastFoodGM(nbases=8, Xdim=300).transform(np.zeros((2, 300)))
