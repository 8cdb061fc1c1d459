"""RadialBasis, SigmoidalBasis and PolynomialBasis children in the resident SVI loops of GeneralizedLinearModel.fit
(``resident_bases="all"``: RR_SGD_CHILD_CENTRES / RR_SGD_CHILD_POLY of rr_glm_sgd) -- against the reference's recorded gradient
of one step (tests/golden/centres.npz, glm.py:205-294 with basis_functions.py:616-815) and against the host loop around
`_elbo`, which tests/test_gpu_centres.py holds to the same golden arrays.  Same seeds -> same minibatches, same draws, same
start point: the two loops must produce the same fit.  Laid out like tests/test_gpu_resident_sgd.py."""
import numpy as np
import pytest

from conftest import normwise

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True, params=["two streams", "one stream"])
def _order_of_work(monkeypatch, request):
    """Every test runs with the loop's second stream and feature matrix (step t + 1's features -- and a centres child's scale
    kernel -- behind step t's length-scale update, under its Ed product) and without."""
    monkeypatch.setenv("RR_GLM_SGD_OVERLAP", "1" if request.param == "two streams" else "0")


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd.btypes import Bound, Parameter, Positive
    from revrand_amd.glm import GeneralizedLinearModel
    return bs, lk, Bound, Parameter, Positive, GeneralizedLinearModel


def _data(lik, N=1200, d=3, seed=4):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, d)
    f = 0.5 * np.sin(X[:, 0]) + 0.2 * X[:, 2]
    if lik == "poisson":
        return X, rs.poisson(np.exp(f)).astype(float), ()
    if lik == "bernoulli":
        return X, (rs.rand(N) < 1 / (1 + np.exp(-3 * f))).astype(float), ()
    if lik == "binomial":
        n = rs.randint(5, 30, size=N).astype(float)
        return X, rs.binomial(n.astype(int), 1 / (1 + np.exp(-3 * f))).astype(float), (n,)
    return X, f + 0.1 * rs.randn(N), ()


def _flat(v):
    if isinstance(v, (list, tuple)):
        return np.concatenate([_flat(u) for u in v]) if len(v) else np.empty(0)
    return np.atleast_1d(np.asarray(v, dtype=float)).ravel()


@pytest.fixture
def spies(monkeypatch):
    """Counts the steps of each kind of loop and the host route's device contractions (FeatureMatrix.glm_centres: one per
    centres child and host-loop step)."""
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


def _fit(make_basis, lik, resident, X, y, largs, batch=300, maxiter=12, K=3, L=8, nstarts=2, devices=None, seen=None,
         resident_bases="all"):
    bs, lk, Bound, Parameter, Positive, GLM = _imports()
    like = {"poisson": lk.Poisson, "bernoulli": lk.Bernoulli, "binomial": lk.Binomial, "gaussian": lk.Gaussian}[lik]()
    glm = GLM(like, make_basis(), K=K, nsamples=L, batch_size=batch, maxiter=maxiter, nstarts=nstarts, random_state=11,
              resident_bases=resident_bases, devices=devices)
    glm._resident_sgd = resident
    if seen is not None:
        seen.update({k: 0 for k in seen if isinstance(seen[k], int)})
    np.random.seed(3)  # (the start point is a draw from NumPy's global stream, as in the reference)
    glm.fit(X, y, likelihood_args=largs)
    return (glm.weights_.copy(), glm.covariance_.copy(), _flat(glm.regularizer_), _flat(glm.like_hypers_), _flat(glm.basis_hypers_),
            glm.random_.randn())


def _same(a, b, tol):
    for u, v in zip(a[:5], b[:5]):
        assert u.shape == v.shape
        if u.size:
            assert normwise(u, v) < tol, (normwise(u, v), tol)
    assert a[5] == b[5]  # the RandomState ends in the same state: same minibatches, same draws consumed


def _worst(a, b):
    return max(normwise(u, v) for u, v in zip(a[:5], b[:5]) if u.size)


_HOST = {}   # host-loop fits, made once per configuration (they do not depend on RR_GLM_SGD_OVERLAP)


def _host_fit(key, seen, *args, **kwargs):
    if key not in _HOST:
        _HOST[key] = _fit(*args, seen=seen, **kwargs)
        assert seen["resident"] == 0 and seen["fused"] == 0   # none of the host loop's steps went through a device loop
    return _HOST[key]


def _centres_basis(kind, ard, X, M=65):
    bs, lk, Bound, Parameter, Positive, GLM = _imports()
    d = X.shape[1]
    cls = bs.RadialBasis if kind == "radial" else bs.SigmoidalBasis
    return lambda: cls(centres=X[:M].copy(), lenscale=Parameter(np.ones(d), Positive()) if ard else Parameter(1.0, Positive()))


# ---- T1: one step against the reference's recorded gradient ------------------------------------------------------------

def test_one_step_against_the_reference_s_gradient(golden):
    """tests/golden/centres.npz glm_*: radial ARD + LinearBasis(onescol=True), N = 64, d = 4, M = 24, F = 29, K = 3, L = 8,
    Bernoulli.  One plain SGD step of rr_glm_sgd on all 64 rows with the reference's draws: (z0 - z1) / eta IS the gradient
    the loop formed -- [-dm | -dC | dL | dbp] of glm.py:238-283 -- and objs[0] the step's -ELBO.  Also pins the sign and the
    1 / l^6 of a radial length scale's gradient (basis_functions.py:712-719)."""
    from revrand_amd import _hip
    from revrand_amd import likelihoods as lk
    g = golden("centres")
    X, y, C, ls = g["glm_X"], g["glm_y"], g["glm_C"], g["glm_ls"]
    N, d = X.shape
    K, L, F = int(g["glm_K"]), int(g["glm_L"]), C.shape[0] + d + 1
    dev = _hip.get_device()
    h = _hip.CentresHandle(C, "radial")
    fm = _hip.FeatureMatrix(N, F)
    dX = dev.upload_matrix(np.ascontiguousarray(X, dtype=np.float32))
    dy = dev.upload_vector(y, np.float32)
    dE = dev.upload_vector(np.ascontiguousarray(g["glm_e"].reshape(K * L, F), dtype=np.float32))
    z0 = np.concatenate([g["glm_m"].ravel(), g["glm_Cv"].ravel(), g["glm_regs"].ravel(), ls.ravel()])
    eta = 1e-3
    sgd = _hip.ResidentSgd(fm, [("centres", h, d), ("linear", d, True)], K, 0, z0, np.full(z0.size, -np.inf),
                           np.full(z0.size, np.inf), np.zeros(z0.size, dtype=bool), _hip.UPDATER_IDS["SGDUpdater"], [eta], 1)
    try:
        view = _hip.DeviceView(dX, 0, N)
        sgd.step([view, view], N, dy, None, lk.RR_LIK_BERNOULLI, 0.0, float(g["glm_B"]), L, dE)
        z1, objs, _ = sgd.read()
    finally:
        sgd.close()
        for b in (dX, dy, dE):
            b.free()
    grad = (z0 - z1) / eta
    fk = F * K
    got = (grad[:fk].reshape(F, K), grad[fk:2 * fk].reshape(F, K), grad[2 * fk:2 * fk + 2], grad[2 * fk + 2:])
    e = (abs(objs[0] - g["glm_obj"]) / abs(g["glm_obj"]), normwise(got[0], g["glm_ndm"]), normwise(got[1], g["glm_ndC"]),
         normwise(got[2], g["glm_dL"]), normwise(got[3], g["glm_dbp"]))
    print("resident step vs reference: obj %.2e dm %.2e dC %.2e dL %.2e dbp %.2e" % e)
    assert got[3].shape == (d,)
    assert all(v < 1e-3 for v in e), e


# ---- T2: resident loop = host loop, one child --------------------------------------------------------------------------

@pytest.mark.parametrize("lik", ["poisson", "gaussian"])
@pytest.mark.parametrize("ard", [True, False], ids=["ard", "isotropic"])
@pytest.mark.parametrize("kind", ["radial", "sigmoid"])
def test_resident_loop_equals_host_loop(kind, ard, lik, spies):
    """65 centres (two centre tiles, the second with one column), minibatches of 300 rows (not a multiple of the 32-row
    sub-tile), 12 Adam steps; the Gaussian's variance sits in front of the length scales in the flat vector."""
    X, y, largs = _data(lik)
    mk = _centres_basis(kind, ard, X)
    dev = _fit(mk, lik, True, X, y, largs, seen=spies)
    assert spies == {"resident": 12, "fused": 0, "glm_centres": 0}
    host = _host_fit(("one", kind, ard, lik), spies, mk, lik, False, X, y, largs)
    assert dev[4].shape == ((3,) if ard else (1,))
    _same(dev, host, 2e-5)


# ---- T3: concatenations -------------------------------------------------------------------------------------------------

def _cat(X, radial_lenscale=None):
    bs, lk, Bound, Parameter, Positive, GLM = _imports()
    d = X.shape[1]

    def make():
        rl = radial_lenscale() if radial_lenscale is not None else Parameter(np.ones(d), Positive())
        return bs.LinearBasis(onescol=True, regularizer=Parameter(0.7, Positive())) \
            + bs.RadialBasis(centres=X[:21].copy(), lenscale=rl, regularizer=Parameter(1.5, Positive())) \
            + bs.RandomRBF(nbases=8, Xdim=d, random_state=1) \
            + bs.PolynomialBasis(order=3, include_bias=False) \
            + bs.SigmoidalBasis(centres=X[30:47, [0, 2]].copy(), apply_ind=[0, 2], lenscale=Parameter(0.8, Positive()))
    return make


@pytest.mark.parametrize("lik", ["binomial", "gaussian"])
def test_concatenation_with_centre_and_polynomial_children(lik, spies):
    """Linear | radial (ARD) | random Fourier | polynomial | sigmoid (isotropic, on two of the three columns of X): every child its
    own regulariser over its column slice; the radial block starts at column 4 (16-byte aligned), the sigmoid block at column
    50 (not aligned: the feature kernel's shifted tile)."""
    X, y, largs = _data(lik)
    mk = _cat(X)
    widths = [int(b.get_dim(X)) for b in mk().bases]
    col0 = np.concatenate([[0], np.cumsum(widths)[:-1]])
    assert widths == [4, 21, 16, 9, 17] and col0[1] & 3 == 0 and col0[4] & 3 != 0
    dev = _fit(mk, lik, True, X, y, largs, seen=spies)
    assert spies == {"resident": 12, "fused": 0, "glm_centres": 0}
    host = _host_fit(("cat", lik), spies, mk, lik, False, X, y, largs)
    assert dev[2].shape == (5,) and dev[4].shape == (3 + 1 + 1,)
    _same(dev, host, 5e-5)


def test_bounded_radial_length_scales_are_truncated_and_clipped(spies):
    """A plain Bound (no log trick) on the radial child's length scales that the optimiser pushes into: sgd.py:404-420."""
    bs, lk, Bound, Parameter, Positive, GLM = _imports()
    X, y, largs = _data("binomial")
    mk = _cat(X, radial_lenscale=lambda: Parameter(np.full(3, 1.0), Bound(0.97, 1.02)))
    dev = _fit(mk, "binomial", True, X, y, largs, seen=spies, maxiter=15)
    assert spies["resident"] == 15
    host = _host_fit(("cat bounded",), spies, mk, "binomial", False, X, y, largs, maxiter=15)
    _same(dev, host, 5e-5)
    rl = dev[4][:3]
    assert np.all(rl >= 0.97) and np.all(rl <= 1.02) and (np.any(rl == 0.97) or np.any(rl == 1.02))


def test_polynomial_basis_alone(spies):
    """No length scale at all: [1 | x_i, x_i^2 per column] -- the loop runs without the length-scale half of its update."""
    bs, lk, Bound, Parameter, Positive, GLM = _imports()
    X, y, largs = _data("gaussian")
    mk = lambda: bs.PolynomialBasis(order=2)  # noqa: E731
    dev = _fit(mk, "gaussian", True, X, y, largs, seen=spies)
    assert spies == {"resident": 12, "fused": 0, "glm_centres": 0}
    host = _host_fit(("poly",), spies, mk, "gaussian", False, X, y, largs)
    assert dev[0].shape == (7, 3) and dev[4].size == 0
    _same(dev, host, 5e-5)


# ---- T4: small minibatches ----------------------------------------------------------------------------------------------

def test_small_minibatches_take_the_step_per_call_loop(spies):
    """12 rows per minibatch: a random Fourier fit of this shape goes to the many-steps-per-launch kernel (rr_svi.hip), which
    does not hold these children -- every step is an rr_glm_sgd_step."""
    bs, lk, Bound, Parameter, Positive, GLM = _imports()
    X, y, largs = _data("poisson")
    d = X.shape[1]
    mk = lambda: bs.RadialBasis(centres=X[:21].copy(), lenscale=Parameter(np.ones(d), Positive())) \
        + bs.LinearBasis(onescol=True) + bs.PolynomialBasis(order=2, include_bias=False)  # noqa: E731
    dev = _fit(mk, "poisson", True, X, y, largs, batch=12, seen=spies)
    assert spies == {"resident": 12, "fused": 0, "glm_centres": 0}
    host = _host_fit(("small",), spies, mk, "poisson", False, X, y, largs, batch=12)
    _same(dev, host, 5e-5)


# ---- T5: three steps ----------------------------------------------------------------------------------------------------

def test_three_steps_agree_to_the_noise_of_the_steps_float32_atomics(spies):
    """Three Adam steps of the radial ARD fit above.  Both loops run the same float32 feature, GEMM and contraction kernels and
    finish in float64 (the loop multiplies the summed S_i by 1 / l^6 once, the host route every block's partial sum: 1e-16);
    what is left is the last-bit noise of the step's float32 K-split atomics times Adam's step length, as for the random
    Fourier children (tests/test_gpu_resident_sgd.py: 1e-9 of the parameters).  The difference between two host-loop runs is
    that floor; both are printed.  Measured on an MI355X: resident vs host 0 (the same bits in every block), host vs host 0 -- at
    this shape no GEMM of the step splits K, and the 1e-16 between the two loops' float64 sums disappears in Adam's normalised
    step.  Both are below 1e-9, so the bound is the project's 1e-8."""
    X, y, largs = _data("poisson")
    mk = _centres_basis("radial", True, X)
    dev = _fit(mk, "poisson", True, X, y, largs, maxiter=3, seen=spies)
    assert spies["resident"] == 3
    host = _host_fit(("three", 0), spies, mk, "poisson", False, X, y, largs, maxiter=3)
    again = _host_fit(("three", 1), spies, mk, "poisson", False, X, y, largs, maxiter=3)
    floor = _worst(again, host)
    print("three steps: resident vs host %.3e, host vs host %.3e" % (_worst(dev, host), floor))
    assert floor < 1e-9   # what makes 1e-8 the bound: the host loop's own run-to-run difference stays below 1e-9
    _same(dev, host, 1e-8)


# ---- T6: the default is unchanged ---------------------------------------------------------------------------------------

def test_default_keeps_centres_fits_on_the_host_loop(monkeypatch):
    """resident_bases left at "fourier": a Radial + Linear fit never reaches a device loop."""
    bs, lk, Bound, Parameter, Positive, GLM = _imports()
    from revrand_amd import _hip
    monkeypatch.setattr(_hip.ResidentSgd, "step", lambda *a, **k: (_ for _ in ()).throw(AssertionError("resident loop used")))
    monkeypatch.setattr(_hip.FusedSvi, "run", lambda *a, **k: (_ for _ in ()).throw(AssertionError("fused loop used")))
    X, y, _ = _data("bernoulli")
    for batch in (300, 12):
        glm = GLM(lk.Bernoulli(), bs.RadialBasis(centres=X[:16].copy()) + bs.LinearBasis(onescol=True), K=2, nsamples=4,
                  batch_size=batch, maxiter=3, nstarts=0, random_state=1)
        assert glm.resident_bases == "fourier"
        glm.fit(X, y)
        assert np.all(np.isfinite(glm.weights_))


# ---- T7: device group ---------------------------------------------------------------------------------------------------

@pytest.fixture
def group_spies(monkeypatch):
    """As tests/test_gpu_resident_group.py: steps per kind of loop, every member's parameters as the group loop leaves them, the
    rows each member got per step; members take part from 256 rows of a minibatch each."""
    from revrand_amd import _hip, multigpu
    monkeypatch.setattr(multigpu.ShardedMinibatchFeatures, "MIN_ROWS_PER_MEMBER", 256)
    seen = {"group": 0, "one": 0, "fused": 0, "z": [], "rows": []}
    real_g, real_1, real_f, real_close = _hip.ResidentSgdGroup.step, _hip.ResidentSgd.step, _hip.FusedSvi.run, _hip.ResidentSgdGroup.close

    def g(self, parts, *a, **k):
        seen["group"] += 1
        seen["rows"].append([p[1] for p in parts])
        return real_g(self, parts, *a, **k)

    def one(self, *a, **k):
        seen["one"] += 1
        return real_1(self, *a, **k)

    def f(self, n, *a, **k):
        seen["fused"] += n
        return real_f(self, n, *a, **k)

    def close(self):
        if all(s.h for s in self.sgds):
            seen["z"].append([s.read()[0] for s in self.sgds])
        return real_close(self)
    monkeypatch.setattr(_hip.ResidentSgdGroup, "step", g)
    monkeypatch.setattr(_hip.ResidentSgd, "step", one)
    monkeypatch.setattr(_hip.FusedSvi, "run", f)
    monkeypatch.setattr(_hip.ResidentSgdGroup, "close", close)
    return seen


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0]])
def test_group_resident_fit_equals_the_one_context_fit(devices, group_spies):
    """Radial (ARD) + linear + polynomial children on every member of a device group: the centres child's sums S_i ride the
    all-reduce of the length-scale contractions, the members' copies of the parameters stay the same bits."""
    bs, lk, Bound, Parameter, Positive, GLM = _imports()
    X, y, largs = _data("poisson", N=6000)
    d = X.shape[1]
    mk = lambda: bs.RadialBasis(centres=X[:40].copy(), lenscale=Parameter(np.ones(d), Positive())) \
        + bs.LinearBasis(onescol=True) + bs.PolynomialBasis(order=2, include_bias=False)  # noqa: E731
    one = _fit(mk, "poisson", True, X, y, largs, batch=1500)
    assert group_spies["one"] == 12 and group_spies["group"] == 0 and group_spies["fused"] == 0
    many = _fit(mk, "poisson", True, X, y, largs, batch=1500, devices=devices)
    assert group_spies["group"] == 12 and group_spies["one"] == 12 and group_spies["fused"] == 0
    assert all(sum(r) == 1500 and len(r) == len(devices) for r in group_spies["rows"])
    zs = group_spies["z"][-1]
    assert len(zs) == len(devices) and all(np.array_equal(z, zs[0]) for z in zs[1:])
    _same(many, one, 2e-5)


# ---- T8: sharded StandardLinearModel ------------------------------------------------------------------------------------

def _elbo_once(SLM, basis, X, y, var, reg, ls, devices=None):
    from revrand_amd import multigpu
    slm = SLM(basis, devices=devices)
    slm.obj_ = -np.inf
    slm._state = slm._make_state(X, y)
    assert slm._state is not None
    assert isinstance(slm._state, multigpu.ShardedFitState) == (devices is not None)
    try:
        f, (gv, gr, gh) = slm._elbo(X, y, var, reg, ls)
        C = slm._state.best_covariance() if getattr(slm._state, "best_on_device", False) else slm.covariance_
    finally:
        slm._state.release()
        slm._state = None
    from revrand_amd.utils import flatten_values
    return np.asarray(flatten_values([f, gv, gr, gh]), dtype=float), slm.weights_, np.array(C)


def test_sharded_slm_elbo_equals_the_one_context_elbo(monkeypatch):
    """StandardLinearModel(RadialBasis + LinearBasis, devices=[0, 0]): the rows on two members (a ShardedFitState, no longer one
    GPU), one `_elbo` -- objective, dvar, dreg, the length scales' gradient -- against one context, to the tolerances
    tests/test_gpu_multigpu.py::test_sharded_elbo_equals_the_one_context_elbo holds random Fourier bases to."""
    bs, lk, Bound, Parameter, Positive, GLM = _imports()
    from revrand_amd import multigpu
    from revrand_amd.slm import StandardLinearModel as SLM
    monkeypatch.setenv("RR_POSDEF", "device")
    rs = np.random.RandomState(3)
    N, d = 2000, 4
    X = rs.randn(N, d)
    y = np.sin(X[:, 0]) + 0.3 * X[:, 1] + 0.1 * rs.randn(N)
    mk = lambda: bs.RadialBasis(centres=X[:24].copy(), lenscale=Parameter(np.ones(d), Positive())) + bs.LinearBasis(onescol=True)  # noqa: E731
    st = multigpu.ShardedFitState.make(mk(), X, y, multigpu.get_group([0, 0]))
    assert st is not None
    st.release()
    ls = np.linspace(0.8, 1.3, d)
    v1, w1, C1 = _elbo_once(SLM, mk(), X, y, 0.3, [1.2, 0.8], ls)
    v, w, C = _elbo_once(SLM, mk(), X, y, 0.3, [1.2, 0.8], ls, devices=[0, 0])
    assert v.shape == v1.shape == (1 + 1 + 2 + d,)
    assert abs(v[0] - v1[0]) < 1e-6 * abs(v1[0]) and normwise(v[1:], v1[1:]) < 1e-4, (v, v1)   # f32 row sums regrouped
    assert normwise(v[-d:], v1[-d:]) < 1e-4, (v[-d:], v1[-d:])   # the centres child's dhyp, tree-summed over the members, on its own
    assert normwise(w, w1) < 2e-4 and normwise(C, C1) < 2e-4


# ---- refusals -----------------------------------------------------------------------------------------------------------

def test_invalid_centre_and_polynomial_records_are_refused_cleanly():
    """rr_glm_sgd_create: RR_ERR_INVALID with a message for a centres child whose n_ls is neither 1 nor d, whose handle computes
    in float64 or lives on another context, and for a polynomial child without a column or with a negative order;
    rr_glm_svi_create (the fused small-minibatch kernel) refuses both kinds -- an error, never a crash."""
    from revrand_amd import _hip
    rs = np.random.RandomState(0)
    d, M, K, N = 3, 5, 2, 40
    C = rs.randn(M, d)
    dev = _hip.get_device()
    h32, h64 = _hip.CentresHandle(C, "radial"), _hip.CentresHandle(C, "sigmoid", compute="f64")
    other = _hip.get_upload_device(dev.index)   # a second context of the same GPU
    with _hip.device_scope(other):
        h_other = _hip.CentresHandle(C, "radial")

    def make(children, F, n_ls):
        np_ = 2 * F * K + len(children) + n_ls
        return _hip.ResidentSgd(_hip.FeatureMatrix(16, F), children, K, 0, np.ones(np_), np.full(np_, -np.inf), np.full(np_, np.inf),
                                np.zeros(np_, dtype=bool), _hip.UPDATER_IDS["Adam"], [1e-2, 0.9, 0.99, 1e-8], 2)
    for children, F, n_ls, word in (([("centres", h32, 2)], M, 2, "centres basis"), ([("centres", h64, d)], M, d, "centres basis"),
                                    ([("centres", h_other, d)], M, d, "centres basis"), ([("poly", d, False, 0)], 1, 0, "polynomial"),
                                    ([("poly", d, True, -1)], 1, 0, "polynomial"), ([("poly", 0, True, 2)], 1, 0, "polynomial")):
        with pytest.raises(_hip.HipError, match=word):
            make(children, F, n_ls)
    make([("centres", h32, d), ("poly", d, True, 0)], M + 1, d).close()   # (valid: a bias column alone is a polynomial of order 0)

    dX = dev.upload_matrix(np.ascontiguousarray(rs.randn(N, d), dtype=np.float32))
    dy = dev.upload_vector(rs.randn(N), np.float32)
    try:
        for child, F, n_ls in ((("centres", h32, d, dX), M, d), (("poly", d, True, 2, dX), 1 + 2 * d, 0)):
            np_ = 2 * F * K + 1 + n_ls
            with pytest.raises(_hip.HipError, match="not taken by the fused loop"):
                _hip.FusedSvi(dev, [child], N, dy, None, None, K, 4, 8, 3, 0, np.ones(np_), np.full(np_, -np.inf), np.full(np_, np.inf),
                              np.zeros(np_, dtype=bool), _hip.UPDATER_IDS["Adam"], [1e-2, 0.9, 0.99, 1e-8], 5, N / 8.0)
    finally:
        dX.free()
        dy.free()
