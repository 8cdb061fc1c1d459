"""RadialBasis, SigmoidalBasis and PolynomialBasis on the MI355X: stand-alone transform / grad, the feature-matrix kernels
at ragged shapes, the concatenated Gram, the resident `_elbo` / fit of StandardLinearModel, the second pass' fixed-order
gradient contraction, predictions, and the GLM step -- against the reference's recorded outputs
(tests/golden/centres*.npz) and the float64 restatement (tests/centres_cases.py).

Tolerances are the project's (tests/test_gpu_rff.py, tests/test_gpu_slm.py): normwise 1e-3 for f32 arithmetic, 1e-5 for f64,
2e-3 for length-scale gradients, 1e-4 relative on the ELBO."""
import types

import numpy as np
import pytest

import centres_cases as cc
import revrand_oracle as orc
from conftest import normwise

pytestmark = pytest.mark.gpu

SHAPES = [(1, 7), (5, 33), (8, 48)]
TAGS = ["iso0.9", "iso1.7", "ard"]
KINDS = ["RadialBasis", "SigmoidalBasis"]
TOL = {"f32": 1e-3, "f64": 1e-5}


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    from revrand_amd.btypes import Parameter, Positive
    from revrand_amd.slm import StandardLinearModel
    return bs, _hip, Parameter, Positive, StandardLinearModel


def lenscale_of(tag, d):
    return {"iso0.9": 0.9, "iso1.7": 1.7}.get(tag, np.linspace(0.7, 1.6, d))


def golden_arrays(golden, name):
    return golden("centres_sigmoid" if name == "SigmoidalBasis" else "centres")


def make_basis(bs, Parameter, Positive, name, C, ard, **kw):
    par = Parameter(np.ones(C.shape[1]), Positive()) if ard else Parameter(1., Positive())
    return getattr(bs, name)(centres=C, lenscale=par, **kw)


def restated(name, X, C, ls, grad=False, budget=1 << 22):
    """cc.TRANSFORM / cc.GRAD in row chunks (the restatement forms an (N, M, d) array)."""
    fn = (cc.GRAD if grad else cc.TRANSFORM)[name]
    step = max(1, budget // max(1, C.shape[0] * C.shape[1]))
    return np.concatenate([fn(X[r:r + step], C, ls) for r in range(0, max(len(X), 1), step)]) if len(X) else fn(X, C, ls)


# ---- stand-alone transform / grad ------------------------------------------------------------------------------------

@pytest.mark.parametrize("xdtype", [np.float32, np.float64])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("d,M", SHAPES)
@pytest.mark.parametrize("name", KINDS)
def test_transform_grad_vs_reference(golden, name, d, M, tag, dtype, xdtype):
    bs, _hip, Parameter, Positive, _ = _imports()
    g, gb = golden("centres"), golden_arrays(golden, name)
    X, C = g["X_d%d" % d], g["C_d%d" % d]
    ls = lenscale_of(tag, d)
    basis = make_basis(bs, Parameter, Positive, name, C, tag == "ard", dtype=dtype)
    Xin = X.astype(xdtype)
    Phi, dPhi = basis.transform(Xin, ls), basis.grad(Xin, ls)
    wantP, wantD = gb["%s_d%d_%s_Phi" % (name, d, tag)], gb["%s_d%d_%s_dPhi" % (name, d, tag)]
    assert Phi.dtype == np.float64 and dPhi.dtype == np.float64 and dPhi.shape == wantD.shape
    tol = TOL[dtype]   # (float32 X is 6e-8 away from the recorded inputs: far inside either bound)
    eP, eD = normwise(Phi, wantP), normwise(dPhi, wantD)
    print("%s d=%d %s %s X%s: Phi %.2e dPhi %.2e" % (name, d, tag, dtype, np.dtype(xdtype).name, eP, eD))
    assert eP < tol and eD < tol


@pytest.mark.parametrize("name", KINDS)
def test_apply_ind_default_lenscale_and_empty_input(name):
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(3)
    X, C = rs.randn(40, 6), rs.randn(9, 3)
    ind = [4, 0, 2]
    basis = getattr(bs, name)(centres=C, lenscale=Parameter(np.array([0.8, 1.1, 1.4]), Positive()), apply_ind=ind)
    ls = basis.params.value
    assert normwise(basis.transform(X), cc.TRANSFORM[name](X[:, ind], C, ls)) < 1e-3   # lenscale=None: the initial value
    assert normwise(basis.grad(X, ls), cc.GRAD[name](X[:, ind], C, ls)) < 1e-3
    # a strided view of wider rows goes through with its leading dimension
    wide = rs.randn(40, 10)
    b3 = getattr(bs, name)(centres=C)
    assert normwise(b3.transform(wide[:, :3], 1.2), cc.TRANSFORM[name](wide[:, :3], C, 1.2)) < 1e-3
    for n in (0, 1):
        Xn = X[:n][:, ind]
        b = getattr(bs, name)(centres=C, lenscale=Parameter(np.ones(3), Positive()))
        assert b.transform(Xn, ls).shape == (n, 9) and b.grad(Xn, ls).shape == (n, 9, 3)
        assert b3.grad(Xn, 1.2).shape == (n, 9)
        if n:
            assert normwise(b.transform(Xn, ls), cc.TRANSFORM[name](Xn, C, ls)) < 1e-3
            assert normwise(b.grad(Xn, ls), cc.GRAD[name](Xn, C, ls)) < 1e-3
            assert normwise(b3.grad(Xn, 1.2), cc.GRAD[name](Xn, C, 1.2)) < 1e-3


# ---- ragged shapes: stand-alone kernels and the feature-matrix kernel ------------------------------------------------

@pytest.mark.parametrize("d", [1, 21, 128])
@pytest.mark.parametrize("M", [1, 63, 65, 300, 1025])
@pytest.mark.parametrize("N", [1, 255, 257, 5000])
@pytest.mark.parametrize("name", KINDS)
def test_ragged_shapes_vs_restatement(name, N, M, d):
    """Any rows, M and col0: the block sits at col0 = 3 between two other children's columns; those, and the padding columns
    of the matrix, are bit for bit what they were."""
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(N + 7 * M + d)
    X, C = rs.randn(N, d), rs.randn(M, d)
    ard = d > 1 and (N + M) % 2 == 1
    base = 1.1 * max(1.0, d ** 0.25) if name == "RadialBasis" else 1.1 * max(1.0, d ** 0.5)   # features of order one
    ls = base * np.linspace(0.8, 1.3, d) if ard else base
    basis = make_basis(bs, Parameter, Positive, name, C, ard)
    want = restated(name, X, C, ls)
    assert normwise(basis.transform(X, ls), want) < 1e-3
    if N * M * (d if ard else 1) * 8 <= (64 << 20):
        assert normwise(basis.grad(X, ls), restated(name, X, C, ls, grad=True)) < 1e-3
    dev = _hip.get_device()
    F = 3 + M + 2
    fm = _hip.FeatureMatrix(N, F)
    fm.begin(N)
    left, right = rs.randn(N, 3).astype(np.float32), rs.randn(N, 2).astype(np.float32)
    fm.put_host(left, 0)
    fm.put_host(right, 3 + M)
    dX = dev.upload_matrix(X.astype(np.float32))
    fm.put_centres(basis._handle(), dX, basis._check_dim(d, ls), 3)
    P = fm.download()
    dX.free()
    assert P.shape == (N, (F + 255) // 256 * 256)
    assert np.array_equal(P[:, :3], left) and np.array_equal(P[:, 3 + M:F], right)
    assert not P[:, F:].any()
    assert normwise(P[:, 3:3 + M], want) < 1e-3


def test_polynomial_features_on_the_device():
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(5)
    dev = _hip.get_device()
    for N, d, order, bias in [(1, 1, 1, True), (257, 5, 3, True), (1000, 7, 4, False), (33, 3, 0, True)]:
        X = rs.randn(N, d)
        want = cc.poly_transform(X, order, bias)
        F = 5 + want.shape[1]
        fm = _hip.FeatureMatrix(N, F)
        fm.begin(N)
        left = rs.randn(N, 5).astype(np.float32)
        fm.put_host(left, 0)
        dX = dev.upload_matrix(X.astype(np.float32))
        fm.put_poly(dX, order, bias, 5)
        P = fm.download()
        dX.free()
        assert np.array_equal(P[:, :5], left) and not P[:, F:].any()
        assert normwise(P[:, 5:F], want) < 1e-5


# ---- concatenated Gram ------------------------------------------------------------------------------------------------

def test_concatenated_gram_vs_float64():
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(12)
    N, d, M = 20000, 6, 70
    X, C = rs.randn(N, d), rs.randn(M, d)
    y = np.sin(X[:, 0]) + 0.1 * rs.randn(N)
    rbf = bs.RandomRBF(nbases=50, Xdim=d, random_state=3)
    cat = bs.RadialBasis(centres=C, lenscale=Parameter(np.ones(d), Positive())) + bs.PolynomialBasis(order=3) + rbf \
        + bs.LinearBasis(onescol=True)
    ls = np.linspace(1.0, 1.6, d)
    Phi = np.hstack((cc.radial_transform(X, C, ls), cc.poly_transform(X, 3), orc.rff_transform(X, rbf.W, 1.3),
                     np.ones((N, 1)), X))
    G, b, yty = cat.gram(X, y, ls, 1.3)
    assert G.shape == (Phi.shape[1],) * 2
    assert normwise(G, Phi.T @ Phi) < 1e-3 and normwise(b, Phi.T @ y) < 1e-3
    assert abs(yty - y @ y) < 1e-3 * (y @ y)
    # the estimator-level transform of the concatenation is the same matrix
    assert normwise(cat.transform(X[:100], ls, 1.3), Phi[:100]) < 1e-3


# ---- StandardLinearModel: the golden _elbo cases and the golden fit ---------------------------------------------------

def _elbo_case(bs, Parameter, Positive, g, tag, dtype):
    C = g["elbo_C"]
    d = C.shape[1]

    def ardp():
        return Parameter(np.ones(d), Positive())
    if tag == "radial_iso":
        return bs.RadialBasis(centres=C, dtype=dtype), float(g["elbo_reg"][0]), float(g["elbo_iso"])
    if tag == "radial_ard":
        return bs.RadialBasis(centres=C, lenscale=ardp(), dtype=dtype), float(g["elbo_reg"][0]), g["elbo_ard"]
    if tag == "sigmoid_ard":
        return bs.SigmoidalBasis(centres=C, lenscale=ardp(), dtype=dtype), float(g["elbo_reg"][0]), g["elbo_ard"]
    cat = bs.RadialBasis(centres=C, lenscale=ardp(), dtype=dtype) + bs.PolynomialBasis(order=2) + bs.LinearBasis()
    return cat, list(g["elbo_reg"]), g["elbo_ard"]


ELBO_TAGS = ["radial_iso", "radial_ard", "sigmoid_ard", "radial_poly_linear"]


def _check_elbo(g, tag, slm, res, tol, tol_elbo, tol_dhyp):
    nelbo, (ndvar, ndreg, ndhyp) = res
    e = dict(elbo=abs(-nelbo - g["elbo_%s_elbo" % tag]) / abs(g["elbo_%s_elbo" % tag]),
             m=normwise(slm.weights_, g["elbo_%s_m" % tag]), C=normwise(slm.covariance_, g["elbo_%s_C" % tag]),
             dvar=normwise(-ndvar, g["elbo_%s_dvar" % tag]), dreg=normwise(-np.atleast_1d(ndreg), g["elbo_%s_dreg" % tag]),
             dhyp=normwise(-np.atleast_1d(ndhyp), g["elbo_%s_dhyp" % tag]))
    print(tag, " ".join("%s %.2e" % kv for kv in e.items()))
    assert np.shape(ndhyp) == (() if tag == "radial_iso" else g["elbo_%s_dhyp" % tag].shape)
    assert e["elbo"] < tol_elbo and e["m"] < tol and e["C"] < tol and e["dvar"] < tol and e["dreg"] < tol
    assert e["dhyp"] < tol_dhyp


@pytest.mark.parametrize("tag", ELBO_TAGS)
def test_elbo_resident_vs_reference(golden, monkeypatch, tag):
    bs, _hip, Parameter, Positive, SLM = _imports()
    g = golden("centres")
    X, y = g["elbo_X"], g["elbo_y"]
    basis, reg, hyp = _elbo_case(bs, Parameter, Positive, g, tag, "f32")

    def no_host_grad(self, *a, **k):
        raise AssertionError("the basis' host grad ran during a resident _elbo")
    monkeypatch.setattr(bs.RadialBasis, "grad", no_host_grad)
    slm = SLM(basis)
    slm.obj_ = -np.inf
    slm._state = slm._make_state(X, y)
    try:
        assert isinstance(slm._state, bs.CatFitState)
        assert any(isinstance(c, bs._ResidentCentres) for c in slm._state.children)
        res = slm._elbo(X, y, float(g["elbo_var"]), reg, hyp)
        nobj = slm._elbo_objective(X, y, float(g["elbo_var"]), reg, hyp)
    finally:
        slm._state.release()
        slm._state = None
    _check_elbo(g, tag, slm, res, 1e-3, 1e-4, 2e-3)
    assert abs(nobj - res[0]) < 1e-4 * abs(res[0])


@pytest.mark.parametrize("tag", ELBO_TAGS)
def test_elbo_f64_bases_take_the_host_route(golden, tag):
    bs, _hip, Parameter, Positive, SLM = _imports()
    g = golden("centres")
    X, y = g["elbo_X"], g["elbo_y"]
    basis, reg, hyp = _elbo_case(bs, Parameter, Positive, g, tag, "f64")
    slm = SLM(basis)
    slm.obj_ = -np.inf
    assert slm._make_state(X, y) is None
    res = slm._elbo(X, y, float(g["elbo_var"]), reg, hyp)
    _check_elbo(g, tag, slm, res, 1e-5, 1e-5, 1e-5)


def test_fit_end_to_end_vs_reference(golden):
    """Same data, centres, fixed initial values, nstarts=0, maxiter=20 as the reference run -- a run that converges (see
    gen_fit of tools/make_centres_golden.py) -- compared at prediction level, as tests/test_gpu_slm.py does: L-BFGS
    trajectories are sensitive to the last bits."""
    bs, _hip, Parameter, Positive, SLM = _imports()
    g = golden("centres")
    X, y, Xs, C = g["fit_X"], g["fit_y"], g["fit_Xs"], g["fit_C"]
    var0, ls0, reg0, reg1 = (float(v) for v in g["fit_start"])
    basis = bs.RadialBasis(centres=C, lenscale=Parameter(ls0, Positive()), regularizer=Parameter(reg0, Positive())) \
        + bs.LinearBasis(onescol=True, regularizer=Parameter(reg1, Positive()))
    made = []
    make = basis.device_fit_state

    def spy(X_, y_):
        made.append(make(X_, y_))
        return made[-1]
    basis.device_fit_state = spy
    slm = SLM(basis, var=Parameter(var0, Positive()), nstarts=0, maxiter=20, random_state=0).fit(X, y)
    assert len(made) == 1 and isinstance(made[0], bs.CatFitState)
    Ey, Vy = slm.predict_moments(Xs)
    smse = ((g["fit_Ey"] - Ey) ** 2).mean() / g["fit_Ey"].var()
    print("fit: smse %.2e Vy %.2e obj %.6f vs %.6f" % (smse, normwise(Vy, g["fit_Vy"]), slm.obj_, float(g["fit_obj"])))
    assert smse < 1e-3
    assert np.all(Vy > 0) and normwise(Vy, g["fit_Vy"]) < 0.2
    assert abs(slm.obj_ - float(g["fit_obj"])) < 0.02 * abs(float(g["fit_obj"]))
    Phi = np.hstack((cc.radial_transform(Xs, C, slm.hypers_), np.ones((len(Xs), 1)), Xs))
    Eo, Vo = orc.slm_predict_moments(Phi, slm.weights_, slm.covariance_, slm.var_)
    assert normwise(Ey, Eo) < 1e-3 and normwise(Vy, Vo) < 1e-3
    assert normwise(slm.predict(Xs), Eo) < 1e-3


# ---- second pass: ragged chunks, fixed-order reduction -----------------------------------------------------------------

# (N, d, M, chunk_rows, the chunks that gives).  d = 128 with ARD length scales is the contraction kernel's largest
# configuration: 128 dimension lanes x 2 slices, 57.5 KB of dynamic LDS, three centre tiles the last of them ragged.
PASS2_SHAPES = {"d21": (5000, 21, 300, 1700, [1667, 1667, 1666]), "d128": (1500, 128, 130, 512, [500, 500, 500])}


@pytest.mark.parametrize("name,ard,shape", [("RadialBasis", True, "d21"), ("RadialBasis", False, "d21"),
                                            ("SigmoidalBasis", True, "d21"), ("RadialBasis", True, "d128"),
                                            ("SigmoidalBasis", True, "d128")])
def test_second_pass_chunked_and_bitwise_reproducible(name, ard, shape):
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(21)
    N, d, M, chunk_rows, chunks = PASS2_SHAPES[shape]
    var = 0.5
    X, C = rs.randn(N, d), rs.randn(M, d)
    y = np.sin(X[:, 0] - X[:, 1]) + 0.1 * rs.randn(N)
    base = {"d21": (2.2, 4.0), "d128": (3.0, 9.0)}[shape][name != "RadialBasis"]   # features of order one
    ls = base * np.linspace(0.9, 1.2, d) if ard else base
    Phi = restated(name, X, C, ls)
    dP = restated(name, X, C, ls, grad=True)
    dPl = [dP[:, :, i] for i in range(d)] if ard else [dP]
    o = orc.slm_elbo(Phi, y, var, np.full(M, 1.3), slice(None), dPl)
    sq = ((y - Phi @ o["m"]) ** 2).sum()
    basis = make_basis(bs, Parameter, Positive, name, C, ard)
    st = bs.CatFitState(types.SimpleNamespace(get_dim=basis.get_dim, bases=[basis]), [bs._ResidentCentres(basis, X)], X, y,
                        chunk_rows=chunk_rows)
    try:
        assert [rows for _, rows in st._chunks()] == chunks
        out = [st.second_pass([ls], o["m"], o["C"], var) for _ in range(2)]
    finally:
        st.release()
    want = -np.atleast_1d(np.array(o["dhyp"], dtype=float))
    got = np.atleast_1d(out[0][1])
    print("%s ard=%s %s: sqErr %.2e dhyp %.2e" % (name, ard, shape, abs(out[0][0] - sq) / sq, normwise(got, want)))
    assert np.shape(out[0][1]) == ((d,) if ard else ())
    assert abs(out[0][0] - sq) < 2e-3 * sq
    assert normwise(got, want) < 2e-3
    assert np.array_equal(np.atleast_1d(out[1][1]), got)   # two fixed-order stages: the same bits every time


@pytest.mark.parametrize("name", KINDS)
def test_float64_device_rows_and_length_scales_recorded_by_the_put(name):
    """The C ABI with a float64 device X (the Python children always upload float32): features, polynomial powers and the
    second pass' contraction read it directly.  And the contraction uses the length scales its block was PUT with: a
    stand-alone transform with other length scales on the same handle in between does not change its result."""
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(71)
    N, d, M, var = 700, 5, 70, 0.4
    X, C = rs.randn(N, d), rs.randn(M, d)
    y = np.sin(X[:, 0]) + 0.1 * rs.randn(N)
    ls = (1.2 if name == "RadialBasis" else 2.0) * np.linspace(0.9, 1.3, d)
    poly = cc.poly_transform(X, 2)
    Phi = np.hstack((poly, cc.TRANSFORM[name](X, C, ls)))
    dP = cc.GRAD[name](X, C, ls)
    col0, F = poly.shape[1], Phi.shape[1]
    dPl = [np.hstack((np.zeros_like(poly), dP[:, :, i])) for i in range(d)]
    o = orc.slm_elbo(Phi, y, var, np.full(F, 1.3), slice(None), dPl)
    basis = make_basis(bs, Parameter, Positive, name, C, True)
    h, dev = basis._handle(), _hip.get_device()
    got = {}
    for xdtype in (np.float64, np.float32):
        dX = dev.upload_matrix(X.astype(xdtype))
        assert dX.dtype == np.dtype(xdtype)
        dy = dev.upload_vector(y.astype(np.float32))
        dg = dev.zeros(d * 8)
        fm = _hip.FeatureMatrix(N, F)
        fm.begin(N)
        fm.put_poly(dX, 2, True, 0)
        fm.put_centres(h, dX, ls, col0)
        assert normwise(fm.download()[:, :F], Phi) < 1e-3
        fm.pass2_begin(o["m"], o["C"])
        fm.pass2_rows(dy)
        assert h.transform(X[:4], 0.7).shape == (4, M)   # isotropic, other value: rewrites the handle's cached factors
        fm.pass2_centres(h, dX, col0, dg)
        with pytest.raises(_hip.HipError, match="was not put at column"):
            fm.pass2_centres(h, dX, col0 - 1, dg)
        fm.pass2_end()
        got[xdtype] = -dev.download(dg, (d,), np.float64) / var
        for buf in (dX, dy, dg):
            buf.free()
    want = -np.array(o["dhyp"], dtype=float)
    print("%s: dhyp f64 X %.2e f32 X %.2e" % (name, normwise(got[np.float64], want), normwise(got[np.float32], want)))
    assert normwise(got[np.float64], want) < 2e-3 and normwise(got[np.float32], want) < 2e-3


# ---- predictions ---------------------------------------------------------------------------------------------------

def test_predict_moments_vs_oracle():
    bs, _hip, Parameter, Positive, SLM = _imports()
    rs = np.random.RandomState(31)
    N, d, M = 3000, 5, 40
    X, C = rs.randn(N, d), rs.randn(M, d)
    cat = bs.SigmoidalBasis(centres=C) + bs.PolynomialBasis(order=2, include_bias=False) \
        + bs.RadialBasis(centres=C, lenscale=Parameter(np.ones(d), Positive())) + bs.LinearBasis()
    hyp = [1.4, np.linspace(0.9, 1.5, d)]
    Phi = np.hstack((cc.sigmoid_transform(X, C, hyp[0]), cc.poly_transform(X, 2, False), cc.radial_transform(X, C, hyp[1]),
                     np.ones((N, 1)), X))
    F = Phi.shape[1]
    A = rs.randn(F, F) / np.sqrt(F)
    slm = SLM(cat)
    slm.weights_, slm.covariance_ = rs.randn(F), A @ A.T + 0.1 * np.eye(F)
    slm.var_, slm.regularizer_, slm.hypers_ = 0.3, [1.0] * 4, hyp
    Ey, Vy = slm.predict_moments(X)
    Eo, Vo = orc.slm_predict_moments(Phi, slm.weights_, slm.covariance_, slm.var_)
    assert normwise(Ey, Eo) < 1e-3 and normwise(Vy, Vo) < 1e-3
    assert normwise(slm.predict(X), Eo) < 1e-3


# ---- GeneralizedLinearModel --------------------------------------------------------------------------------------------

def test_glm_minibatch_elbo_vs_reference(golden, monkeypatch):
    bs, _hip, Parameter, Positive, _ = _imports()
    from revrand_amd import likelihoods as lk
    from revrand_amd.glm import GeneralizedLinearModel as GLM
    g = golden("centres")
    X, y, C, ls = g["glm_X"], g["glm_y"], g["glm_C"], g["glm_ls"]
    d = X.shape[1]
    basis = bs.RadialBasis(centres=C, lenscale=Parameter(np.ones(d), Positive())) + bs.LinearBasis(onescol=True)
    glm = GLM(likelihood=lk.Bernoulli(), basis=basis, K=int(g["glm_K"]), nsamples=int(g["glm_L"]), random_state=int(g["glm_seed"]))
    glm.B_, glm.D_ = float(g["glm_B"]), C.shape[0] + d + 1
    glm._GeneralizedLinearModel__it = -1
    # the estimator's seeded stream gives the draws the reference recorded
    K, L, D = int(g["glm_K"]), int(g["glm_L"]), C.shape[0] + d + 1
    e = np.random.RandomState(int(g["glm_seed"])).randn(K * L, D)
    assert np.array_equal(np.stack([e[k * L:(k + 1) * L] for k in range(K)]), g["glm_e"])

    def no_host_grad(self, *a, **k):
        raise AssertionError("the basis' host grad ran during a GLM step")
    monkeypatch.setattr(bs.RadialBasis, "grad", no_host_grad)
    nobj, (ndm, ndC, dL, dlp, dbp) = glm._elbo(g["glm_m"].copy(), g["glm_Cv"].copy(), list(g["glm_regs"]), [], [ls], X, y)
    glm._release_features()
    e = (abs(nobj - g["glm_obj"]) / abs(g["glm_obj"]), normwise(ndm, g["glm_ndm"]), normwise(ndC, g["glm_ndC"]),
         normwise(np.array(dL, dtype=float), g["glm_dL"]), normwise(np.atleast_1d(dbp), g["glm_dbp"]))
    print("glm: obj %.2e dm %.2e dC %.2e dL %.2e dbp %.2e" % e)
    assert np.shape(dbp) == (d,) and dlp == []
    assert all(v < 1e-3 for v in e)


def test_glm_fit_uses_the_device_contraction(monkeypatch):
    bs, _hip, Parameter, Positive, _ = _imports()
    from revrand_amd import likelihoods as lk
    from revrand_amd.glm import GeneralizedLinearModel as GLM
    rs = np.random.RandomState(41)
    N, d, M = 600, 2, 16
    X = rs.randn(N, d)
    p = 1 / (1 + np.exp(-3 * np.sin(2 * X[:, 0])))
    y = (rs.rand(N) < p).astype(float)
    basis = bs.RadialBasis(centres=X[:M].copy()) + bs.LinearBasis(onescol=True)
    calls = {"centres": 0}
    real = _hip.FeatureMatrix.glm_centres

    def counting(self, *a, **k):
        calls["centres"] += 1
        return real(self, *a, **k)

    def no_edphi(self, *a, **k):
        raise AssertionError("the host-gradient branch (glm_edphi) ran for a centres child")
    monkeypatch.setattr(_hip.FeatureMatrix, "glm_centres", counting)
    monkeypatch.setattr(_hip.FeatureMatrix, "glm_edphi", no_edphi)
    glm = GLM(likelihood=lk.Bernoulli(), basis=basis, K=2, maxiter=200, batch_size=50, nsamples=10, nstarts=0, random_state=1)
    glm.fit(X, y)
    assert calls["centres"] >= 100   # one contraction per step of the host loop
    Ey = glm.predict(X)
    assert Ey.shape == (N,) and np.all(np.isfinite(Ey)) and np.all((Ey >= 0) & (Ey <= 1))
    glm._release_features()


# ---- guards ------------------------------------------------------------------------------------------------------------

def test_put_over_claimed_columns_is_refused():
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(51)
    X, C = rs.randn(64, 3), rs.randn(10, 3)
    basis = bs.RadialBasis(centres=C)
    dev = _hip.get_device()
    dX = dev.upload_matrix(X.astype(np.float32))
    fm = _hip.FeatureMatrix(64, 16)
    fm.begin(64)
    fm.put_linear(dX, True, 0)   # columns [0, 4)
    with pytest.raises(_hip.HipError, match="overlap"):
        fm.put_centres(basis._handle(), dX, np.array([1.0]), 2)
    with pytest.raises(_hip.HipError, match="overlap"):
        fm.put_poly(dX, 2, True, 3)
    with pytest.raises(_hip.HipError, match="out of range"):
        fm.put_centres(basis._handle(), dX, np.array([1.0]), 8)
    fm.put_centres(basis._handle(), dX, np.array([1.0]), 4)
    with pytest.raises(_hip.HipError, match="overlap"):
        fm.put_centres(basis._handle(), dX, np.array([1.0]), 4)
    # a random Fourier entry point does not take a centres handle, nor the other way round
    with pytest.raises(_hip.HipError):
        fm.put_rff(basis._handle(), dX, np.array([1.0]), 14)
    rff = bs.RandomRBF(nbases=1, Xdim=3, random_state=0)
    with pytest.raises(_hip.HipError):
        fm.put_centres(rff._handle(), rff._handle().upload(X.astype(np.float32)), np.array([1.0]), 14)
    dX.free()


def test_wide_inputs_fall_back_to_the_generic_child():
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(61)
    N, d, M = 700, 130, 20
    X, C = rs.randn(N, d), rs.randn(M, d)
    y = rs.randn(N)
    radial = bs.RadialBasis(centres=C)
    assert radial._resident_child(X) is None and radial.device_fit_state(X, y) is None
    cat = radial + bs.LinearBasis(onescol=False, apply_ind=[0, 1])
    Phi = np.hstack((restated("RadialBasis", X, C, 4.0), X[:, :2]))
    G, b, _ = cat.gram(X, y, 4.0)
    assert normwise(G, Phi.T @ Phi) < 1e-3 and normwise(b, Phi.T @ y) < 1e-3
    feats = bs.MinibatchFeatures(cat)
    feats.assemble(X, [4.0])
    assert type(feats.children[0][0]) is bs._ResidentGeneric
    assert normwise(feats.fm.download()[:, :M + 2], Phi) < 1e-3
    feats.release()
    assert normwise(radial.grad(X, 4.0), restated("RadialBasis", X, C, 4.0, grad=True)) < 1e-3
