"""RadialBasis, SigmoidalBasis and PolynomialBasis in the FLOAT64 device feature matrix (rr_featmat64_put_centres / put_poly /
pass2_centres / download) and the float64 resident fit they give StandardLinearModel(resident_bases="all") -- against the
float64 restatement (tests/centres_cases.py), the NumPy oracle and the reference's recorded outputs (tests/golden/centres.npz).

Tolerances, all normwise (conftest.normwise):
* features 1e-12: z is a sum of d <= 128 squared differences, relative error <= (d + 2) 2^-53 ~ 1.5e-14; with z <~ 1.3 for
  the length scales used here and one exp that is <~ 2e-14 in Phi.  1e-12 is 50x that, four orders below float32.
* the length scales' gradient 1e-10: for the inputs of CONTRACT_CASES the conditioning |sum|E o dPhi_i|| / |sum E o dPhi_i| of
  the sums is <= 87 and two float64 evaluation orders of the same sums differ by <= 3.8e-14
  (test_contraction_inputs_stay_within_the_tolerance recomputes both on the CPU -- in the max norm over the length scales it
  finds <= 56 and <= 3.2e-14 -- and caps them at 100 and 1e-12); rounding only Phi and Phi C to float32 moves
  the result by 2.8e-10 .. 1.5e-8.  1e-10 is 2500x the float64 disagreement and below the smallest float32 effect.
* the golden `_elbo` cases 1e-5, the project's float64 contract (tests/test_gpu_centres.py holds the host route to it)."""
import functools
import types

import numpy as np
import pytest

import centres_cases as cc
import revrand_oracle as orc
from conftest import normwise

KINDS = ["RadialBasis", "SigmoidalBasis"]
gpu = pytest.mark.gpu


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    from revrand_amd.btypes import Parameter, Positive
    from revrand_amd.slm import StandardLinearModel
    return bs, _hip, Parameter, Positive, StandardLinearModel


def make_basis(bs, Parameter, Positive, name, C, ard, **kw):
    par = Parameter(np.ones(C.shape[1]), Positive()) if ard else Parameter(1., Positive())
    return getattr(bs, name)(centres=C, lenscale=par, **kw)


def restated(name, X, C, ls, grad=False, budget=1 << 22):
    """cc.TRANSFORM / cc.GRAD in row chunks (the restatement forms an (N, M, d) array)."""
    fn = (cc.GRAD if grad else cc.TRANSFORM)[name]
    step = max(1, budget // max(1, C.shape[0] * C.shape[1]))
    return np.concatenate([fn(X[r:r + step], C, ls) for r in range(0, len(X), step)])


def rounded(X, xdtype):
    """What the device reads: the inputs after the upload's rounding, as float64."""
    return X.astype(xdtype).astype(np.float64)


# ---- 1. feature blocks: ragged shapes, both store alignments, neighbours and padding intact ---------------------------------

@gpu
@pytest.mark.parametrize("d", [1, 21, 128])
@pytest.mark.parametrize("M", [1, 63, 65, 130])
@pytest.mark.parametrize("N", [1, 255, 257])
@pytest.mark.parametrize("name", KINDS)
def test_feature_blocks_ragged_neighbours_intact(name, N, M, d):
    """The block at col0 = 3 and 4 (both parities of the two-double store) between two other children's columns, from float32 and
    float64 device rows: the neighbours are bit for bit what they were, the padding columns [F, ld) stay zero."""
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(N + 7 * M + d)
    X, C = rs.randn(N, d), rs.randn(M, d)
    ard = d > 1 and (N + M) % 2 == 1
    base = 1.1 * max(1.0, d ** 0.25) if name == "RadialBasis" else 1.1 * max(1.0, d ** 0.5)   # features of order one
    ls = base * np.linspace(0.8, 1.3, d) if ard else base
    basis = make_basis(bs, Parameter, Positive, name, C, ard, dtype="f64")
    dev = _hip.get_device()
    for xdtype in (np.float64, np.float32):
        want = restated(name, rounded(X, xdtype), C, ls)
        dX = dev.upload_matrix(X.astype(xdtype))
        assert dX.dtype == np.dtype(xdtype)
        for col0 in (3, 4):
            F = col0 + M + 2
            fm = _hip.FeatureMatrix64(N, F)
            fm.begin(N)
            left, right = rs.randn(N, col0), rs.randn(N, 2)
            fm.put_host(left, 0)
            fm.put_host(right, col0 + M)
            fm.put_centres(basis._handle(), dX, basis._check_dim(d, ls), col0)
            P = fm.download()
            assert P.dtype == np.float64 and P.shape == (N, (F + 127) // 128 * 128)
            assert np.array_equal(P[:, :col0], left) and np.array_equal(P[:, col0 + M:F], right)
            assert not P[:, F:].any()
            e = normwise(P[:, col0:col0 + M], want)
            print("%s N=%d M=%d d=%d X%s col0=%d: %.2e" % (name, N, M, d, np.dtype(xdtype).name, col0, e))
            assert e < 1e-12
        dX.free()


@gpu
def test_polynomial_features_in_the_float64_matrix():
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(5)
    dev = _hip.get_device()
    for N, d, order, bias in [(1, 1, 1, True), (257, 5, 3, True), (1000, 7, 4, False), (33, 3, 0, True)]:
        X = rs.randn(N, d)
        for xdtype in (np.float64, np.float32):
            want = cc.poly_transform(rounded(X, xdtype), order, bias)
            F = 5 + want.shape[1] + 2
            fm = _hip.FeatureMatrix64(N, F)
            fm.begin(N)
            left, right = rs.randn(N, 5), rs.randn(N, 2)
            fm.put_host(left, 0)
            fm.put_host(right, F - 2)
            dX = dev.upload_matrix(X.astype(xdtype))
            fm.put_poly(dX, order, bias, 5)
            P = fm.download()
            dX.free()
            assert np.array_equal(P[:, :5], left) and np.array_equal(P[:, F - 2:F], right) and not P[:, F:].any()
            assert normwise(P[:, 5:F - 2], want) < 1e-12


# ---- 2. the contraction: ragged chunks, fixed-order reduction -----------------------------------------------------------------

# (N, d, M, chunk_rows, the chunks that gives).  Three centre tiles of 32 at d21 is not enough to leave one ragged: M = 130 gives
# five, the last of two centres; d = 128 with ARD length scales is the kernel's largest LDS configuration.
PASS2_SHAPES = {"d21": (1200, 21, 130, 500, [400, 400, 400]), "d128": (600, 128, 70, 256, [200, 200, 200])}
CONTRACT_CASES = [("RadialBasis", True, "d21"), ("RadialBasis", False, "d21"), ("SigmoidalBasis", True, "d21"),
                  ("RadialBasis", True, "d128"), ("SigmoidalBasis", True, "d128")]
# the isotropic d128 inputs as well: no GPU case, but the figures the tolerance was derived from cover them
INPUT_CASES = CONTRACT_CASES + [("RadialBasis", False, "d128"), ("SigmoidalBasis", False, "d128")]
VAR = 0.5


@functools.lru_cache(maxsize=None)
def contract_case(name, ard, shape):
    """The inputs of tests/test_gpu_centres.py::test_second_pass_chunked_and_bitwise_reproducible at this file's shapes, with the
    oracle's posterior and gradient, made once and shared (read-only) by the GPU test and the CPU check of the inputs."""
    rs = np.random.RandomState(21)
    N, d, M, chunk_rows, chunks = PASS2_SHAPES[shape]
    X, C = rs.randn(N, d), rs.randn(M, d)
    y = np.sin(X[:, 0] - X[:, 1]) + 0.1 * rs.randn(N)
    base = {"d21": (2.2, 4.0), "d128": (3.0, 9.0)}[shape][name != "RadialBasis"]   # features of order one
    ls = base * np.linspace(0.9, 1.2, d) if ard else base
    Phi = restated(name, X, C, ls)
    dP = restated(name, X, C, ls, grad=True)
    dPl = [dP[:, :, i] for i in range(d)] if ard else [dP]
    o = orc.slm_elbo(Phi, y, VAR, np.full(M, 1.3), slice(None), dPl)
    err = y - Phi @ o["m"]
    E = np.outer(err, o["m"]) - Phi @ o["C"]
    direct = np.array([(E * g).sum() for g in dPl]) / VAR          # a second float64 evaluation order of the same sums
    absum = np.array([np.abs(E * g).sum() for g in dPl]) / VAR
    for a in (X, C, y, o["m"], o["C"]):
        a.setflags(write=False)
    return dict(X=X, C=C, y=y, ls=ls, m=o["m"], Cpost=o["C"], sq=(err ** 2).sum(), dhyp=np.array(o["dhyp"], dtype=float),
                direct=direct, cond=np.abs(absum).max() / np.abs(direct).max(), chunk_rows=chunk_rows, chunks=chunks, d=d)


@pytest.mark.parametrize("name,ard,shape", INPUT_CASES)
def test_contraction_inputs_stay_within_the_tolerance(name, ard, shape):
    """No device: the two figures the 1e-10 of the GPU test rests on, recomputed from the restatement for its inputs."""
    c = contract_case(name, ard, shape)
    dis = normwise(c["direct"], c["dhyp"])
    print("%s ard=%s %s: conditioning %.1f, order disagreement %.2e" % (name, ard, shape, c["cond"], dis))
    assert c["cond"] <= 100
    assert dis <= 1e-12


@gpu
@pytest.mark.parametrize("name,ard,shape", CONTRACT_CASES)
def test_second_pass_chunked_and_bitwise_reproducible(name, ard, shape):
    bs, _hip, Parameter, Positive, _ = _imports()
    c = contract_case(name, ard, shape)
    X, y, d = c["X"], c["y"], c["d"]
    basis = make_basis(bs, Parameter, Positive, name, c["C"], ard, dtype="f64")
    child = bs._ResidentCentres(basis, X, "f64")
    assert child.dX.dtype == np.float64
    st = bs.CatFitState(types.SimpleNamespace(get_dim=basis.get_dim, bases=[basis]), [child], X, y, chunk_rows=c["chunk_rows"],
                        dtype="f64")
    try:
        assert [rows for _, rows in st._chunks()] == c["chunks"]
        out = [st.second_pass([c["ls"]], c["m"], c["Cpost"], VAR) for _ in range(2)]
    finally:
        st.release()
    want = -np.atleast_1d(c["dhyp"])
    got = np.atleast_1d(out[0][1])
    print("%s ard=%s %s: sqErr %.2e dhyp %.2e" % (name, ard, shape, abs(out[0][0] - c["sq"]) / c["sq"], normwise(got, want)))
    assert np.shape(out[0][1]) == ((d,) if ard else ())
    assert abs(out[0][0] - c["sq"]) < 1e-12 * c["sq"]
    assert normwise(got, want) < 1e-10
    assert np.array_equal(np.atleast_1d(out[1][1]), got)   # two fixed-order stages: the same bits every time


# ---- 3. the C ABI flow: float32 / float64 rows, length scales recorded by the put, refusals ---------------------------------

@gpu
@pytest.mark.parametrize("name", KINDS)
def test_device_rows_and_length_scales_recorded_by_the_put(name):
    """put_poly then put_centres, the second pass, and the contraction with the length scales its block was PUT with: a stand-alone
    transform with other length scales on the same handle in between does not change its result.  Float32 rows are held to the
    oracle evaluated on the rounded inputs; the bounds are this file's (features 1e-12, gradient 1e-10: the conditioning of
    these sums, asserted below, is within the 100 the bound allows for)."""
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(71)
    N, d, M, var = 700, 5, 70, 0.4
    X, C = rs.randn(N, d), rs.randn(M, d)
    y = np.sin(X[:, 0]) + 0.1 * rs.randn(N)
    ls = (1.2 if name == "RadialBasis" else 2.0) * np.linspace(0.9, 1.3, d)
    basis = make_basis(bs, Parameter, Positive, name, C, True, dtype="f64")
    h, dev = basis._handle(), _hip.get_device()
    for xdtype in (np.float64, np.float32):
        Xr = rounded(X, xdtype)
        poly = cc.poly_transform(Xr, 2)
        Phi = np.hstack((poly, cc.TRANSFORM[name](Xr, C, ls)))
        dP = cc.GRAD[name](Xr, C, ls)
        col0, F = poly.shape[1], Phi.shape[1]
        dPl = [np.hstack((np.zeros_like(poly), dP[:, :, i])) for i in range(d)]
        o = orc.slm_elbo(Phi, y, var, np.full(F, 1.3), slice(None), dPl)
        E = np.outer(y - Phi @ o["m"], o["m"]) - Phi @ o["C"]
        cond = max(np.abs(E * g).sum() for g in dPl) / max(abs((E * g).sum()) for g in dPl)
        assert cond <= 100, cond
        dX = dev.upload_matrix(X.astype(xdtype))
        assert dX.dtype == np.dtype(xdtype)
        dy = dev.upload_vector(y)
        dg = dev.zeros(d * 8)
        fm = _hip.FeatureMatrix64(N, F)
        fm.begin(N)
        fm.put_poly(dX, 2, True, 0)
        with pytest.raises(_hip.HipError, match="overlap"):
            fm.put_centres(h, dX, ls, col0 - 1)
        with pytest.raises(_hip.HipError, match="out of range"):
            fm.put_centres(h, dX, ls, col0 + 1)
        fm.put_centres(h, dX, ls, col0)
        with pytest.raises(_hip.HipError, match="overlap"):
            fm.put_centres(h, dX, ls, col0)
        with pytest.raises(_hip.HipError, match="overlap"):
            fm.put_poly(dX, 2, True, 1)
        assert normwise(fm.download()[:, :F], Phi) < 1e-12
        fm.pass2_begin(o["m"], o["C"])
        fm.pass2_rows(dy)
        assert h.transform(X[:4], 0.7).shape == (4, M)   # isotropic, other value: rewrites the handle's cached factors
        fm.pass2_centres(h, dX, col0, dg)
        with pytest.raises(_hip.HipError, match="was not put at column"):
            fm.pass2_centres(h, dX, col0 - 1, dg)
        sq = fm.pass2_end()
        got = -dev.download(dg, (d,), np.float64) / var
        for buf in (dX, dy, dg):
            buf.free()
        want = -np.array(o["dhyp"], dtype=float)
        sqw = ((y - Phi @ o["m"]) ** 2).sum()
        print("%s X%s: conditioning %.1f sqErr %.2e dhyp %.2e" % (name, np.dtype(xdtype).name, cond, abs(sq - sqw) / sqw,
                                                                 normwise(got, want)))
        assert abs(sq - sqw) < 1e-12 * sqw
        assert normwise(got, want) < 1e-10


# ---- 4. StandardLinearModel(resident_bases="all"): the golden _elbo cases ---------------------------------------------------

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


def _check_elbo(g, tag, slm, res, tol):
    nelbo, (ndvar, ndreg, ndhyp) = res
    e = dict(elbo=abs(-nelbo - g["elbo_%s_elbo" % tag]) / abs(g["elbo_%s_elbo" % tag]),
             m=normwise(slm.weights_, g["elbo_%s_m" % tag]), C=normwise(slm.covariance_, g["elbo_%s_C" % tag]),
             dvar=normwise(-ndvar, g["elbo_%s_dvar" % tag]), dreg=normwise(-np.atleast_1d(ndreg), g["elbo_%s_dreg" % tag]),
             dhyp=normwise(-np.atleast_1d(ndhyp), g["elbo_%s_dhyp" % tag]))
    print(tag, " ".join("%s %.2e" % kv for kv in e.items()))
    assert np.shape(ndhyp) == (() if tag == "radial_iso" else g["elbo_%s_dhyp" % tag].shape)
    assert all(v < tol for v in e.values()), e


@gpu
@pytest.mark.parametrize("tag", ELBO_TAGS)
def test_elbo_f64_resident_vs_reference(golden, monkeypatch, tag):
    bs, _hip, Parameter, Positive, SLM = _imports()
    g = golden("centres")
    X, y = g["elbo_X"], g["elbo_y"]
    basis, reg, hyp = _elbo_case(bs, Parameter, Positive, g, tag, "f64")
    assert SLM(basis)._make_state(X, y) is None   # default routing: the host route, as before

    def no_host(self, *a, **k):
        raise AssertionError("the basis' host transform / grad ran during a resident _elbo")
    monkeypatch.setattr(bs.RadialBasis, "grad", no_host)
    monkeypatch.setattr(bs.RadialBasis, "transform", no_host)
    slm = SLM(basis, resident_bases="all")
    slm.obj_ = -np.inf
    slm._state = slm._make_state(X, y)
    try:
        assert isinstance(slm._state, bs.CatFitState) and slm._state.dtype == "f64"
        assert any(isinstance(c, bs._ResidentCentres) for c in slm._state.children)
        if tag == "radial_poly_linear":
            assert any(isinstance(c, bs._ResidentPoly) for c in slm._state.children)
        res = slm._elbo(X, y, float(g["elbo_var"]), reg, hyp)
        nobj = slm._elbo_objective(X, y, float(g["elbo_var"]), reg, hyp)
    finally:
        slm._state.release()
        slm._state = None
    _check_elbo(g, tag, slm, res, 1e-5)
    assert abs(nobj - res[0]) < 1e-9 * abs(res[0])


# ---- 5. a mixed float64 state ---------------------------------------------------------------------------------------------------

@gpu
def test_mixed_float64_state_statistics():
    """A float64 random Fourier child makes the state float64; the f32 RadialBasis, the polynomial and the linear child are
    evaluated in float64 inside it.  The statistics are sums of N products of order-one features: conditioning 1."""
    bs, _hip, Parameter, Positive, SLM = _imports()
    rs = np.random.RandomState(81)
    N, d, M = 700, 6, 30
    X, C = rs.randn(N, d), rs.randn(M, d)
    y = np.sin(X[:, 0]) + 0.1 * rs.randn(N)
    rbf = bs.RandomRBF(nbases=20, Xdim=d, dtype="f64", random_state=3)
    cat = rbf + bs.RadialBasis(centres=C, lenscale=Parameter(np.ones(d), Positive())) + bs.PolynomialBasis(2) \
        + bs.LinearBasis(onescol=True)
    hyp = [1.3, np.linspace(1.0, 1.6, d)]
    Phi = np.hstack((orc.rff_transform(X, rbf.W, hyp[0]), cc.radial_transform(X, C, hyp[1]), cc.poly_transform(X, 2),
                     np.ones((N, 1)), X))
    assert SLM(cat)._make_state(X, y) is None
    st = SLM(cat, resident_bases="all")._make_state(X, y)
    try:
        assert isinstance(st, bs.CatFitState) and st.dtype == "f64"
        kinds = [type(c) for c in st.children]
        assert kinds == [bs._ResidentRFF, bs._ResidentCentres, bs._ResidentPoly, bs._ResidentLinear]
        assert all(c.dX.dtype == np.float64 for c in st.children[1:])
        G, b, yty = st.gram(hyp)
    finally:
        st.release()
    e = (normwise(G, Phi.T @ Phi), normwise(b, Phi.T @ y), abs(yty - y @ y) / (y @ y))
    print("mixed: G %.2e b %.2e yty %.2e" % e)
    assert G.shape == (Phi.shape[1],) * 2 and all(v < 1e-10 for v in e)


# ---- 6. a fit -------------------------------------------------------------------------------------------------------------------

@gpu
def test_fit_end_to_end_vs_reference(golden):
    """tests/test_gpu_centres.py::test_fit_end_to_end_vs_reference with dtype="f64" on the radial child under
    resident_bases="all": one float64 CatFitState for the whole fit, the same prediction-level assertions."""
    bs, _hip, Parameter, Positive, SLM = _imports()
    g = golden("centres")
    X, y, Xs, C = g["fit_X"], g["fit_y"], g["fit_Xs"], g["fit_C"]
    var0, ls0, reg0, reg1 = (float(v) for v in g["fit_start"])
    basis = bs.RadialBasis(centres=C, lenscale=Parameter(ls0, Positive()), regularizer=Parameter(reg0, Positive()), dtype="f64") \
        + bs.LinearBasis(onescol=True, regularizer=Parameter(reg1, Positive()))
    made = []
    make = basis.device_fit_state

    def spy(X_, y_, **kw):
        made.append(make(X_, y_, **kw))
        return made[-1]
    basis.device_fit_state = spy
    slm = SLM(basis, var=Parameter(var0, Positive()), nstarts=0, maxiter=20, random_state=0, resident_bases="all").fit(X, y)
    assert len(made) == 1 and isinstance(made[0], bs.CatFitState) and made[0].dtype == "f64"
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


# ---- 7. two members on one GPU ----------------------------------------------------------------------------------------------

def _elbo_once(SLM, basis, X, y, var, reg, hyp, **kw):
    from revrand_amd.utils import flatten_values
    slm = SLM(basis, resident_bases="all", **kw)
    slm.obj_ = -np.inf
    slm._state = slm._make_state(X, y)
    assert slm._state is not None
    try:
        f, grads = slm._elbo(X, y, var, reg, hyp)
    finally:
        state, slm._state = slm._state, None
        state.release()
    return state, np.asarray(flatten_values([f] + list(grads)), dtype=float)


@gpu
def test_two_members_on_one_gpu(golden):
    bs, _hip, Parameter, Positive, SLM = _imports()
    from revrand_amd import multigpu
    g = golden("centres")
    X, y = g["elbo_X"], g["elbo_y"]
    var = float(g["elbo_var"])
    basis, reg, hyp = _elbo_case(bs, Parameter, Positive, g, "radial_ard", "f64")
    st1, v1 = _elbo_once(SLM, basis, X, y, var, reg, hyp)
    basis, reg, hyp = _elbo_case(bs, Parameter, Positive, g, "radial_ard", "f64")
    st2, v2 = _elbo_once(SLM, basis, X, y, var, reg, hyp, devices=[0, 0])
    assert isinstance(st1, bs.CatFitState) and isinstance(st2, multigpu.ShardedFitState)
    assert all(isinstance(s, bs.CatFitState) and s.dtype == "f64" for s in st2.states)
    assert v1.shape == v2.shape == (1 + 1 + 1 + len(hyp),)
    # the value, dvar and dreg each relative, the length scales' gradient normwise
    e = [abs(v2[k] - v1[k]) / abs(v1[k]) for k in range(3)] + [normwise(v2[3:], v1[3:])]
    print("two members: elbo %.2e dvar %.2e dreg %.2e dhyp %.2e" % tuple(e))
    assert max(e) < 1e-9
