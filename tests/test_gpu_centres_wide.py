"""RadialBasis and SigmoidalBasis on inputs of more than 128 columns as DEVICE children (``resident_bases="all"``): the
dimension-blocked feature kernels of the float32 and the float64 matrix (rr_centres_features_wide_kernel /
rr_centres_features64_wide_kernel), the length-scale contraction in blocks of 128 length scales, StandardLinearModel's resident
`_elbo` and GeneralizedLinearModel's resident SVI loops -- against the float64 restatement (tests/centres_cases.py), the NumPy
oracle's second pass, the narrow (d <= 128) kernels and the default routing's host route.

Length scales follow tests/test_gpu_centres.py's rule, base 1.1 d^(1/4) (radial) / 1.1 d^(1/2) (sigmoid) times
linspace(0.8, 1.3, d): Phi stays in 0.58 .. 0.83 for d = 129 .. 1000.

Tolerances, all normwise (conftest.normwise), are the project's own: Phi 1e-3 in the float32 matrix and 1e-12 in the float64 one
(the rounding of z grows as (d + 2) 2^-24 resp. 2^-53 times z, z <~ 1.7: more than 10x margin at d = 1000), length-scale
gradients 2e-3 (f32) and 1e-10 (f64, tests/test_gpu_centres_f64.py), the golden `_elbo` figure 1e-5 for a dtype="f64" basis.
Where two kernels must run the SAME chain of operations the comparison is `array_equal`."""
import functools
import types

import numpy as np
import pytest

import centres_cases as cc
import revrand_oracle as orc
from conftest import normwise

pytestmark = pytest.mark.gpu

KINDS = ["RadialBasis", "SigmoidalBasis"]
VAR = 0.5


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    from revrand_amd.btypes import Parameter, Positive
    from revrand_amd.slm import StandardLinearModel
    return bs, _hip, Parameter, Positive, StandardLinearModel


def make_basis(bs, Parameter, Positive, name, C, ard, **kw):
    par = Parameter(np.ones(C.shape[1]), Positive()) if ard else Parameter(1., Positive())
    return getattr(bs, name)(centres=C, lenscale=par, **kw)


def lenscales(name, d, ard):
    base = 1.1 * max(1.0, d ** 0.25) if name == "RadialBasis" else 1.1 * max(1.0, d ** 0.5)   # features of order one
    return base * np.linspace(0.8, 1.3, d) if ard else base


def restated(name, X, C, ls, grad=False, budget=1 << 22):
    """cc.TRANSFORM / cc.GRAD in row chunks (the restatement forms an (N, M, d) array)."""
    fn = (cc.GRAD if grad else cc.TRANSFORM)[name]
    step = max(1, budget // max(1, C.shape[0] * C.shape[1]))
    return np.concatenate([fn(X[r:r + step], C, ls) for r in range(0, len(X), step)])


def rounded(X, xdtype):
    """What the device reads: the inputs after the upload's rounding, as float64."""
    return X.astype(xdtype).astype(np.float64)


def put32(_hip, h, X, xdtype, ls, col0=0, neighbours=None):
    """The block of `h` in a float32 matrix at col0 (between `neighbours` = (left, right) host blocks); the downloaded matrix."""
    N, M = X.shape[0], h.M
    left, right = neighbours if neighbours is not None else (np.empty((N, 0), np.float32),) * 2
    assert left.shape[1] == col0
    F = col0 + M + right.shape[1]
    fm = _hip.FeatureMatrix(N, F)
    fm.begin(N)
    if left.shape[1]:
        fm.put_host(left, 0)
    if right.shape[1]:
        fm.put_host(right, col0 + M)
    dX = h.dev.upload_matrix(X.astype(xdtype))
    assert dX.dtype == np.dtype(xdtype)
    fm.put_centres(h, dX, np.atleast_1d(np.asarray(ls, dtype=float)), col0)
    P = fm.download()
    dX.free()
    return P, F


def put64(_hip, h, X, xdtype, ls, col0=0, neighbours=None):
    N, M = X.shape[0], h.M
    left, right = neighbours if neighbours is not None else (np.empty((N, 0)),) * 2
    assert left.shape[1] == col0
    F = col0 + M + right.shape[1]
    fm = _hip.FeatureMatrix64(N, F)
    fm.begin(N)
    if left.shape[1]:
        fm.put_host(left, 0)
    if right.shape[1]:
        fm.put_host(right, col0 + M)
    dX = h.dev.upload_matrix(X.astype(xdtype))
    assert dX.dtype == np.dtype(xdtype)
    fm.put_centres(h, dX, np.atleast_1d(np.asarray(ls, dtype=float)), col0)
    P = fm.download()
    dX.free()
    return P, F


# ---- 1. ragged shapes against the restatement -----------------------------------------------------------------------------

def _ragged(name, N, M, d):
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(N + 7 * M + d)
    X, C = rs.randn(N, d), rs.randn(M, d)
    for ard in (True, False):
        ls = lenscales(name, d, ard)
        basis = make_basis(bs, Parameter, Positive, name, C, ard)
        h = basis._handle()
        lsv = basis._check_dim(d, ls)
        for xdtype in (np.float32, np.float64):
            # the float32 matrix: col0 = 3 between two other children's columns
            want = restated(name, X, C, ls)
            left, right = rs.randn(N, 3).astype(np.float32), rs.randn(N, 2).astype(np.float32)
            P, F = put32(_hip, h, X, xdtype, lsv, 3, (left, right))
            assert P.shape == (N, (F + 255) // 256 * 256)
            assert np.array_equal(P[:, :3], left) and np.array_equal(P[:, 3 + M:F], right)
            assert not P[:, F:].any()
            e32 = normwise(P[:, 3:3 + M], want)
            # the float64 matrix: both parities of the two-double store
            want = restated(name, rounded(X, xdtype), C, ls)
            e64 = []
            for col0 in (3, 4):
                left, right = rs.randn(N, col0), rs.randn(N, 2)
                P, F = put64(_hip, h, X, xdtype, lsv, col0, (left, right))
                assert P.dtype == np.float64 and P.shape == (N, (F + 127) // 128 * 128)
                assert np.array_equal(P[:, :col0], left) and np.array_equal(P[:, col0 + M:F], right)
                assert not P[:, F:].any()
                e64.append(normwise(P[:, col0:col0 + M], want))
            print("%s N=%d M=%d d=%d ard=%s X%s: f32 %.2e f64 %.2e %.2e" % (name, N, M, d, ard, np.dtype(xdtype).name, e32,
                                                                          e64[0], e64[1]))
            assert e32 < 1e-3
            assert max(e64) < 1e-12


@pytest.mark.parametrize("d", [129, 130, 257, 300])
@pytest.mark.parametrize("M", [1, 65, 130])
@pytest.mark.parametrize("N", [1, 77, 300])
@pytest.mark.parametrize("name", KINDS)
def test_ragged_shapes_vs_restatement(name, N, M, d):
    """ARD and isotropic, float32 and float64 device rows, the block between two other children's columns (col0 = 3; the
    float64 matrix also col0 = 4): neighbours and padding bit for bit what they were."""
    _ragged(name, N, M, d)


@pytest.mark.parametrize("name", KINDS)
def test_ragged_shape_at_d_1000(name):
    """Eight dimension blocks, the last of 104."""
    _ragged(name, 300, 70, 1000)


# ---- 2. one live dimension ------------------------------------------------------------------------------------------------

def _one_live(d, istar, N, M, seed):
    """Every column but `istar` holds ONE constant, in every row of X and of C: those differences are exactly zero."""
    rs = np.random.RandomState(seed)
    a = rs.randn(d).astype(np.float32).astype(np.float64)   # (float32 values: float32 rows against float64 centres stay equal)
    X, C = np.tile(a, (N, 1)), np.tile(a, (M, 1))
    X[:, istar], C[:, istar] = rs.randn(N), rs.randn(M)
    return X, C, rs


LIVE = sorted({(d, i) for d in (257, 1000) for i in (0, 127, 128, 129, 255, 256, d - 1)})


@pytest.mark.parametrize("d,istar", LIVE)
@pytest.mark.parametrize("name", KINDS)
def test_one_live_dimension_equals_the_one_dimensional_basis(name, d, istar):
    """A dimension dropped (or counted twice) at a block edge moves Phi by far less than 1e-3 of its norm at d = 1000; here it
    would leave Phi at exactly exp(0) / sigmoid(0), or change the one term there is.  The block must be the d = 1 basis' --
    centres C[:, i*], the scalar length scale ls[i*], rows X[:, i*] -- bit for bit, in both matrices."""
    bs, _hip, Parameter, Positive, _ = _imports()
    N, M = 77, 70
    X, C, _ = _one_live(d, istar, N, M, 1000 * d + istar)
    ls = lenscales(name, d, True)
    wide = make_basis(bs, Parameter, Positive, name, C, True)._handle()
    one = make_basis(bs, Parameter, Positive, name, C[:, [istar]].copy(), False)._handle()
    for put, xdtype in ((put32, np.float32), (put64, np.float64)):
        Pw, _ = put(_hip, wide, X, xdtype, ls)
        P1, _ = put(_hip, one, X[:, [istar]].copy(), xdtype, ls[istar])
        assert len(np.unique(P1[:, :M])) > M   # (the live dimension shows)
        assert np.array_equal(Pw[:, :M], P1[:, :M])


# ---- 3. padding changes no bit ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("extra", [9, 130])
@pytest.mark.parametrize("name", KINDS)
def test_constant_columns_behind_128_change_no_bit(name, extra):
    """X (N, 128), C (M, 128) random, then `extra` columns that hold one constant each in every row and every centre: the wide
    kernel's Phi is the narrow d = 128 kernel's, bit for bit -- one chain t = (x - c) s; z = fma(t, t, z) per (row, centre) in
    ascending dimension order, whatever the block size (a NumPy emulation of the float32 chain gives the same identity)."""
    bs, _hip, Parameter, Positive, _ = _imports()
    rs = np.random.RandomState(300 + extra)
    N, M = 77, 70
    X, C = rs.randn(N, 128), rs.randn(M, 128)
    a = rs.randn(extra).astype(np.float32).astype(np.float64)   # (float32 values: equal in float32 rows and float64 centres)
    Xw, Cw = np.hstack((X, np.tile(a, (N, 1)))), np.hstack((C, np.tile(a, (M, 1))))
    ls = lenscales(name, 128, True)
    lsw = np.concatenate((ls, np.linspace(0.7, 2.0, extra)))
    narrow = make_basis(bs, Parameter, Positive, name, C, True)._handle()
    wide = make_basis(bs, Parameter, Positive, name, Cw, True)._handle()
    for put, xdtype in ((put32, np.float32), (put64, np.float64), (put32, np.float64), (put64, np.float32)):
        Pn, _ = put(_hip, narrow, X, xdtype, ls)
        Pw, _ = put(_hip, wide, Xw, xdtype, lsw)
        assert len(np.unique(Pn[:, :M])) > M
        assert np.array_equal(Pw[:, :M], Pn[:, :M])


# ---- 4. the second pass: ragged chunks, fixed-order reduction ----------------------------------------------------------------

PASS2_SHAPES = {"d130": (700, 130, 70), "d300": (600, 300, 130)}   # (N, d, M), each in three chunks (chunk_rows = 256)
CONTRACT_CASES = [(n, a, s) for s in ("d130", "d300") for n, a in (("RadialBasis", True), ("SigmoidalBasis", True),
                                                                   ("RadialBasis", False))]


@functools.lru_cache(maxsize=None)
def contract_case(name, ard, shape):
    """Inputs, the oracle's posterior and its gradient; made once, shared read-only by the float32 and the float64 test."""
    rs = np.random.RandomState(21)
    N, d, M = PASS2_SHAPES[shape]
    X, C = rs.randn(N, d), rs.randn(M, d)
    y = np.sin(X[:, 0] - X[:, 1]) + 0.1 * rs.randn(N)
    ls = lenscales(name, d, ard)
    Phi = restated(name, X, C, ls)
    dP = restated(name, X, C, ls, grad=True)
    dPl = [dP[:, :, i] for i in range(d)] if ard else [dP]
    o = orc.slm_elbo(Phi, y, VAR, np.full(M, 1.3), slice(None), dPl)
    for a in (X, C, y, o["m"], o["C"]):
        a.setflags(write=False)
    return dict(X=X, C=C, y=y, ls=ls, m=o["m"], Cpost=o["C"], sq=((y - Phi @ o["m"]) ** 2).sum(),
                dhyp=np.array(o["dhyp"], dtype=float), d=d)


def _second_pass(name, ard, shape, dtype, tol_sq, tol):
    bs, _hip, Parameter, Positive, _ = _imports()
    c = contract_case(name, ard, shape)
    X, y, d = c["X"], c["y"], c["d"]
    basis = make_basis(bs, Parameter, Positive, name, c["C"], ard, dtype=dtype)
    child = bs._ResidentCentres(basis, X, "f64") if dtype == "f64" else bs._ResidentCentres(basis, X)
    assert child.dX.dtype == (np.float64 if dtype == "f64" else np.float32)
    st = bs.CatFitState(types.SimpleNamespace(get_dim=basis.get_dim, bases=[basis]), [child], X, y, chunk_rows=256, dtype=dtype)
    try:
        chunks = [rows for _, rows in st._chunks()]
        assert len(chunks) == 3 and sum(chunks) == len(X) and all(r % 32 for r in chunks)
        out = [st.second_pass([c["ls"]], c["m"], c["Cpost"], VAR) for _ in range(2)]
    finally:
        st.release()
    want = -np.atleast_1d(c["dhyp"])
    got = np.atleast_1d(out[0][1])
    print("%s ard=%s %s %s: sqErr %.2e dhyp %.2e" % (name, ard, shape, dtype, abs(out[0][0] - c["sq"]) / c["sq"],
                                                    normwise(got, want)))
    assert np.shape(out[0][1]) == ((d,) if ard else ())
    assert abs(out[0][0] - c["sq"]) < tol_sq * c["sq"]
    assert normwise(got, want) < tol
    assert np.array_equal(np.atleast_1d(out[1][1]), got)   # two fixed-order stages per block of length scales: the same bits


@pytest.mark.parametrize("name,ard,shape", CONTRACT_CASES)
def test_second_pass_chunked_and_bitwise_reproducible(name, ard, shape):
    _second_pass(name, ard, shape, "f32", 2e-3, 2e-3)


@pytest.mark.parametrize("name,ard,shape", CONTRACT_CASES)
def test_second_pass_float64_chunked_and_bitwise_reproducible(name, ard, shape):
    _second_pass(name, ard, shape, "f64", 1e-12, 1e-10)


# ---- 5. one live dimension, contraction ------------------------------------------------------------------------------------

@pytest.mark.parametrize("istar", [0, 127, 128, 129, 255, 256])
@pytest.mark.parametrize("dtype", ["f32", "f64"])
@pytest.mark.parametrize("name", KINDS)
def test_one_live_dimension_contraction(name, dtype, istar):
    """The gradient of the one live length scale against the restatement; every other entry is a sum of exact zeros, so a
    length scale that landed in the wrong slot of its block of 128 shows."""
    bs, _hip, Parameter, Positive, _ = _imports()
    d, N, M = 257, 300, 70
    X, C, rs = _one_live(d, istar, N, M, 5000 + istar)
    y = np.sin(X[:, istar]) + 0.1 * rs.randn(N)
    ls = lenscales(name, d, True)
    Phi = restated(name, X, C, ls)
    dP = restated(name, X, C, ls, grad=True)[:, :, istar]
    o = orc.slm_elbo(Phi, y, VAR, np.full(M, 1.3), slice(None), [dP])
    want = -float(o["dhyp"][0])
    basis = make_basis(bs, Parameter, Positive, name, C, True, dtype=dtype)
    child = bs._ResidentCentres(basis, X, "f64") if dtype == "f64" else bs._ResidentCentres(basis, X)
    st = bs.CatFitState(types.SimpleNamespace(get_dim=basis.get_dim, bases=[basis]), [child], X, y, dtype=dtype)
    try:
        got = np.asarray(st.second_pass([ls], o["m"], o["C"], VAR)[1])
    finally:
        st.release()
    assert got.shape == (d,) and want != 0.0
    print("%s %s i*=%d: %.3e vs %.3e (%.2e)" % (name, dtype, istar, got[istar], want, abs(got[istar] - want) / abs(want)))
    assert abs(got[istar] - want) < 2e-3 * abs(want)
    rest = np.delete(got, istar)
    assert np.all(rest == 0.0), np.nonzero(rest)


# ---- 6. StandardLinearModel._elbo ---------------------------------------------------------------------------------------------

def _elbo_once(SLM, basis, X, y, var, reg, hyp, expect_state, **kw):
    from revrand_amd.utils import flatten_values
    slm = SLM(basis, **kw)
    slm.obj_ = -np.inf
    slm._state = slm._make_state(X, y)
    assert (slm._state is not None) == expect_state
    try:
        f, (gv, gr, gh) = slm._elbo(X, y, var, reg, hyp)
    finally:
        if slm._state is not None:
            slm._state.release()
            slm._state = None
    return float(f), [np.asarray(flatten_values([g]), dtype=float) for g in (gv, gr, gh)]


@pytest.mark.parametrize("dtype,tol", [("f32", 2e-3), ("f64", 1e-5)])
def test_slm_elbo_resident_equals_the_default_route(monkeypatch, dtype, tol):
    """RadialBasis(d = 130, ARD) + LinearBasis: under resident_bases="all" a device-resident `_elbo` (no host grad: no
    (N, M, d) tensor), under the default the host route; objective and every gradient agree."""
    bs, _hip, Parameter, Positive, SLM = _imports()
    rs = np.random.RandomState(91)
    N, d, M = 700, 130, 40
    X, C = rs.randn(N, d), rs.randn(M, d)
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rs.randn(N)
    ls = lenscales("RadialBasis", d, True)
    calls = {"grad": 0}
    real = _hip.CentresHandle.grad

    def counting(self, *a, **k):
        calls["grad"] += 1
        return real(self, *a, **k)
    monkeypatch.setattr(_hip.CentresHandle, "grad", counting)

    def mk():
        return bs.RadialBasis(centres=C, lenscale=Parameter(np.ones(d), Positive()), dtype=dtype) + bs.LinearBasis(onescol=True)
    f1, g1 = _elbo_once(SLM, mk(), X, y, 0.3, [1.2, 0.8], [ls], True, resident_bases="all")
    assert calls["grad"] == 0
    f0, g0 = _elbo_once(SLM, mk(), X, y, 0.3, [1.2, 0.8], [ls], False)
    assert calls["grad"] >= 1
    e = [abs(f1 - f0) / abs(f0)] + [normwise(a, b) for a, b in zip(g1, g0)]
    print("%s: objective %.2e dvar %.2e dreg %.2e dhyp %.2e" % ((dtype,) + tuple(e)))
    assert g1[2].shape == g0[2].shape == (d,)
    assert max(e) < tol, e


# ---- 7. GeneralizedLinearModel: the resident SVI loops -----------------------------------------------------------------------

GLM_TOL = 2e-5


def _glm_data(lik, N=1200, d=130, seed=4):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, d)
    f = 0.5 * np.sin(X[:, 0]) + 0.2 * X[:, 2]
    if lik == "poisson":
        return X, rs.poisson(np.exp(f)).astype(float)
    return X, f + 0.1 * rs.randn(N)


def _flat(v):
    if isinstance(v, (list, tuple)):
        return np.concatenate([_flat(u) for u in v]) if len(v) else np.empty(0)
    return np.atleast_1d(np.asarray(v, dtype=float)).ravel()


@pytest.fixture
def spies(monkeypatch):
    """tests/test_gpu_centres_loop.py's: the steps of each kind of loop, the host route's device contractions."""
    from revrand_amd import _hip
    seen = {"resident": 0, "fused": 0, "glm_centres": 0}
    real_1, real_f, real_c = _hip.ResidentSgd.step, _hip.FusedSvi.run, _hip.FeatureMatrix.glm_centres

    def one(self, *a, **k):
        seen["resident"] += 1
        return real_1(self, *a, **k)

    def f(self, n, *a, **k):
        seen["fused"] += n
        return real_f(self, n, *a, **k)

    def c(self, *a, **k):
        seen["glm_centres"] += 1
        return real_c(self, *a, **k)
    monkeypatch.setattr(_hip.ResidentSgd, "step", one)
    monkeypatch.setattr(_hip.FusedSvi, "run", f)
    monkeypatch.setattr(_hip.FeatureMatrix, "glm_centres", c)
    return seen


def _glm_basis(X, M=65):
    bs, _hip, Parameter, Positive, _ = _imports()
    d = X.shape[1]
    return lambda: bs.RadialBasis(centres=X[:M].copy(), lenscale=Parameter(lenscales("RadialBasis", d, True), Positive())) \
        + bs.LinearBasis(onescol=True)


def _glm_fit(mk, lik, resident, X, y, resident_bases, batch=300, maxiter=12, devices=None):
    from revrand_amd import likelihoods as lk
    from revrand_amd.glm import GeneralizedLinearModel as GLM
    like = {"poisson": lk.Poisson, "gaussian": lk.Gaussian}[lik]()
    glm = GLM(like, mk(), K=3, nsamples=8, batch_size=batch, maxiter=maxiter, nstarts=2, random_state=11,
              resident_bases=resident_bases, devices=devices)
    glm._resident_sgd = resident
    np.random.seed(3)  # (the start point is a draw from NumPy's global stream, as in the reference)
    glm.fit(X, y)
    return (glm.weights_.copy(), glm.covariance_.copy(), _flat(glm.regularizer_), _flat(glm.like_hypers_), _flat(glm.basis_hypers_),
            glm.random_.randn())


def _same(a, b, tol):
    worst = 0.0
    for u, v in zip(a[:5], b[:5]):
        assert u.shape == v.shape
        if u.size:
            worst = max(worst, normwise(u, v))
    print("worst normwise difference %.3e (bound %.1e)" % (worst, tol))
    assert worst < tol, (worst, tol)
    assert a[5] == b[5]  # the RandomState ends in the same state: same minibatches, same draws consumed


@functools.lru_cache(maxsize=None)
def _host_fit(lik):
    """The host-loop fit under default routing, made once per likelihood and shared by the parametrisations that compare against
    it (it does not depend on RR_GLM_SGD_OVERLAP).  It counts its own steps, whichever test asks first: none of them may go
    through a device loop."""
    from unittest import mock
    from revrand_amd import _hip
    X, y = _glm_data(lik)

    def no_device_loop(*a, **k):
        raise AssertionError("a device loop ran under default routing")
    with mock.patch.object(_hip.ResidentSgd, "step", no_device_loop), mock.patch.object(_hip.FusedSvi, "run", no_device_loop):
        return _glm_fit(_glm_basis(X), lik, False, X, y, "fourier")


@pytest.mark.parametrize("overlap", ["1", "0"], ids=["two streams", "one stream"])
@pytest.mark.parametrize("lik", ["poisson", "gaussian"])
def test_glm_resident_loop_equals_the_default_host_loop(lik, overlap, spies, monkeypatch):
    """Radial ARD (d = 130: two dimension blocks, the second of two length scales; M = 65) + linear, minibatches of 300 rows, 12
    Adam steps: every step is a resident one, and the fit is the host loop's under default routing (the generic child:
    `transform` uploaded, the (300, 65, 130) gradient contracted on the host) -- same minibatches, same draws.

    The bound: float32 feature error grows with d, so the resident-vs-host difference was first measured at the widest input
    both routes had before this kernel existed -- the same data cut to 128 columns, on an MI355X: 1.8e-16 (Poisson) and
    2.1e-16 (Gaussian) normwise, worst block (m: 0, C: 2.3e-17, the length scales: 1.8e-16 / 2.1e-16; the host loop against
    itself: 0) -- both loops run the same kernels there.  That is below 1e-5, so the bound is the 2e-5 of
    tests/test_gpu_centres_loop.py; a figure above 1e-5 would have made it twice the figure."""
    monkeypatch.setenv("RR_GLM_SGD_OVERLAP", overlap)
    X, y = _glm_data(lik)
    mk = _glm_basis(X)
    dev = _glm_fit(mk, lik, True, X, y, "all")
    assert spies == {"resident": 12, "fused": 0, "glm_centres": 0}
    assert dev[4].shape == (130,)
    _same(dev, _host_fit(lik), GLM_TOL)


@pytest.mark.parametrize("lik", ["poisson", "gaussian"])
def test_glm_bound_s_premise_at_128_columns(lik):
    """What GLM_TOL rests on, measured again on every run: on the same data cut to 128 columns -- where the resident loop and
    the host loop existed before the wide kernels and run the same narrow kernels -- the two fits differ by less than 1e-5
    (1.8e-16 / 2.1e-16 when the bound was chosen).  The figure is printed."""
    X, y = _glm_data(lik)
    X = np.ascontiguousarray(X[:, :128])
    mk = _glm_basis(X)
    dev = _glm_fit(mk, lik, True, X, y, "all")
    host = _glm_fit(mk, lik, False, X, y, "fourier")
    worst = max(normwise(u, v) for u, v in zip(dev[:5], host[:5]) if u.size)
    print("%s, 128 columns: resident vs host %.3e" % (lik, worst))
    assert worst < 1e-5 and dev[5] == host[5]


def test_glm_group_resident_fit_equals_the_one_context_fit(monkeypatch):
    """devices=[0, 0], members from 256 rows of a minibatch each, minibatches of 1500 rows: the wide child's 130 sums ride the
    all-reduce of the length-scale contractions."""
    from revrand_amd import _hip, multigpu
    monkeypatch.setattr(multigpu.ShardedMinibatchFeatures, "MIN_ROWS_PER_MEMBER", 256)
    seen = {"group": 0, "one": 0}
    real_g, real_1 = _hip.ResidentSgdGroup.step, _hip.ResidentSgd.step

    def g(self, *a, **k):
        seen["group"] += 1
        return real_g(self, *a, **k)

    def one(self, *a, **k):
        seen["one"] += 1
        return real_1(self, *a, **k)
    monkeypatch.setattr(_hip.ResidentSgdGroup, "step", g)
    monkeypatch.setattr(_hip.ResidentSgd, "step", one)
    X, y = _glm_data("poisson", N=6000)
    mk = _glm_basis(X, M=40)
    single = _glm_fit(mk, "poisson", True, X, y, "all", batch=1500)
    assert seen == {"group": 0, "one": 12}
    many = _glm_fit(mk, "poisson", True, X, y, "all", batch=1500, devices=[0, 0])
    assert seen == {"group": 12, "one": 12}
    _same(many, single, GLM_TOL)


# ---- 8. refusal ------------------------------------------------------------------------------------------------------------

def test_more_than_4096_columns_are_refused():
    bs, _hip, Parameter, Positive, _ = _imports()
    h = _hip.CentresHandle(np.zeros((1, 4097)), "radial")
    dX = h.dev.upload_matrix(np.zeros((4, 4097), dtype=np.float32))
    try:
        for fm in (_hip.FeatureMatrix(4, 1), _hip.FeatureMatrix64(4, 1)):
            fm.begin(4)
            with pytest.raises(_hip.HipError, match="4096"):
                fm.put_centres(h, dX, np.array([1.0]), 0)
    finally:
        dX.free()
