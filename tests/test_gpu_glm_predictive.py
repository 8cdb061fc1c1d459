"""`GeneralizedLinearModel(predict_engine="device")`: the likelihood's Ey / loglike / cdf per latent sample, the reductions over
the samples and the quantile bisection on the GPU (rr_featmat_predictive, revrand_amd/csrc/rr_predictive.hip) --
  1. against the reference's recorded prediction surface (tests/golden/glm_predict.npz), at the project's tolerances;
  2. against the host engine on the same latent samples, all five likelihood ids, ragged shapes;
  3. the likelihoods' device functions alone (rr_lik_eval) against the scipy calls revrand_amd/likelihoods.py makes;
  4. row chunks and row shards against the one-call result, bit for bit.
Every figure is printed before it is asserted (run with -s to see them); docs/KERNELS.md 3.35 records the measured ones."""
import numpy as np
import pytest

from conftest import normwise

pytestmark = pytest.mark.gpu

# ---- bounds --------------------------------------------------------------------------------------------------------
# Device engine against host engine (test 2), as (Ey, Vy, logpdf, cdf: normwise; Gaussian interval: relative to max(1, |q|)):
# 16 x the largest difference measured on an MI355X over all cases of the test, rounded up to one digit (docs/KERNELS.md 3.35
# has the measured values).  The margin is for compiler and ROCm drift -- the kernels are deterministic.  None is looser than
# the project's tolerance for the same quantity against the reference (test 1: 1e-5, Vy 1e-4, Gaussian interval 1e-4).
# With two or more samples both engines read the same float32 latent samples, and libm and the order of the sums are all
# that differs.  With ONE sample the host engine's rr_featmat_project forms f as a dot product per row and the device
# engine through the GEMM (by design: every statistic is taken over FSt's columns): two float32 summation orders, ~2e-7 apart, which is then what is measured.
BOUNDS = (6e-15, 6e-15, 2e-14, 5e-14, 3e-14)          # measured 3.7e-16, 3.3e-16, 7.1e-16, 2.8e-15, 1.4e-15
BOUNDS_ONE_SAMPLE = (5e-6, 0.0, 5e-6, 9e-6, 1e-5)     # measured 2.96e-7, 0 (asserted exactly), 2.90e-7, 5.23e-7, 6.11e-7
# The special functions alone (test 3): 16 x measured; the CDF bound has to stay below 1e-9 absolute -- three decades under
# the 1e-6 step margin the count intervals of test 2 rely on.
BOUND_CDF_ABS = 4e-12      # measured 2.3e-13 (binomial, n = 10000; Poisson 9.3e-15, Gaussian 1.1e-16, Bernoulli 0)
BOUND_LOGLIKE_REL = 4e-9   # measured 2.4e-10 (Poisson at mu = 1e6, where y f - mu - gammaln(y + 1) cancels seven digits)
BOUND_EY_REL = 4e-15       # measured 2.1e-16
STEP_MARGIN = 1e-6         # the host's sampled CDF at every integer step must keep this distance from the tail probabilities

LIKS = ["gaussian", "bernoulli", "binomial", "poisson_exp", "poisson_softplus"]


def _say(name, value):
    print("MEASURED %s %.3e" % (name, value))
    return value


def _likelihood(name):
    from revrand_amd import likelihoods as lk
    return {"gaussian": lk.Gaussian, "bernoulli": lk.Bernoulli, "binomial": lk.Binomial,
            "poisson_exp": lambda: lk.Poisson("exp"), "poisson_softplus": lambda: lk.Poisson("softplus")}[name]()


def _model(name, engine, d=3, nbases=20, K=3, devices=None, scale=0.3):
    """A LinearBasis + RandomRBF model whose fitted attributes are set (as the golden test sets them)."""
    import revrand_amd.basis_functions as bs
    from revrand_amd.glm import GeneralizedLinearModel
    basis = bs.LinearBasis(onescol=True) + bs.RandomRBF(nbases=nbases, Xdim=d, random_state=8)
    D = 1 + d + 2 * nbases
    rs = np.random.RandomState(11)
    glm = GeneralizedLinearModel(_likelihood(name), basis, K=K, random_state=0, predict_engine=engine, devices=devices)
    glm.weights_, glm.covariance_ = scale * rs.randn(D, K), 0.02 * rs.rand(D, K) + 1e-3
    glm.regularizer_, glm.basis_hypers_ = [1.0, 1.0], 1.1
    glm.like_hypers_ = 0.3 if name == "gaussian" else []
    return glm


def _data(name, N, d=3, seed=5):
    """(X, y, likelihood_args): targets inside each likelihood's support, a binomial n per row."""
    rs = np.random.RandomState(seed)
    X = rs.randn(N, d)
    nbin = rs.randint(1, 30, size=N).astype(float)
    y = {"gaussian": rs.randn(N), "bernoulli": rs.randint(0, 2, size=N).astype(float),
         "binomial": np.floor(rs.rand(N) * (nbin + 1)), "poisson_exp": rs.poisson(2.0, size=N).astype(float),
         "poisson_softplus": rs.poisson(2.0, size=N).astype(float)}[name]
    return X, y, ((nbin,) if name == "binomial" else ())


def _seeded(glm, fn, *a, **k):
    glm.random_ = np.random.RandomState(77)
    return fn(*a, **k)


def _rel_q(a, b):
    """largest |a - b| / max(1, |b|); a NaN pattern that differs is infinitely far"""
    a, b = np.asarray(a), np.asarray(b)
    if not np.array_equal(np.isnan(a), np.isnan(b)):
        return np.inf
    ok = ~np.isnan(b)
    return float((np.abs(a[ok] - b[ok]) / np.maximum(1.0, np.abs(b[ok]))).max()) if ok.any() else 0.0


# ---- 1. against the reference itself -----------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", ["gaussian", "poisson_exp", "binomial"])
def test_device_prediction_surface_vs_reference(golden, lik):
    """test_prediction_surface_vs_reference of test_gpu_glm.py with predict_engine="device": N = 40, S = 50, K = 3, the
    reference's draws, at the same tolerances.  (From the golden `fs`: the sampled CDF at every integer step of the 12 interval
    rows is at least 3.3e-5 (Poisson) / 1.5e-3 (binomial) away from 0.05 and 0.95, so no rounding difference moves a count
    quantile to another step and no row is left out.)"""
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd.glm import GeneralizedLinearModel
    g = golden("glm_predict")
    X, K, S = g["X"], int(g["K"]), int(g["S"])
    d = X.shape[1]
    basis = bs.LinearBasis(onescol=True) + bs.RandomRBF(nbases=g["W"].shape[1], Xdim=d, random_state=8)
    assert np.array_equal(basis.bases[1].W, g["W"])
    like = {"gaussian": lk.Gaussian, "poisson_exp": lambda: lk.Poisson("exp"), "binomial": lk.Binomial}[lik]()
    glm = GeneralizedLinearModel(like, basis, K=K, random_state=0, predict_engine="device")
    glm.weights_, glm.covariance_, glm.regularizer_ = g["m"], g["C"], [1.0, 1.0]
    glm.like_hypers_ = 0.3 if lik == "gaussian" else []
    glm.basis_hypers_ = float(g["ls"])
    largs = (g["nbin"],) if lik == "binomial" else ()

    Ey, Vy = _seeded(glm, glm.predict_moments, X, S, likelihood_args=largs)
    assert _say("ref_Ey_" + lik, normwise(Ey, g[lik + "_Ey"])) < 1e-5
    assert _say("ref_Vy_" + lik, normwise(Vy, g[lik + "_Vy"])) < 1e-4
    assert normwise(_seeded(glm, glm.predict, X, S, likelihood_args=largs), g[lik + "_Ey"]) < 1e-5
    lp = _seeded(glm, glm.predict_logpdf, X, g["yq_" + lik], S, likelihood_args=largs)
    assert _say("ref_logpdf_" + lik, normwise(np.array(lp), g[lik + "_logpdf"])) < 1e-5
    cdf = _seeded(glm, glm.predict_cdf, X, float(g[lik + "_q"]), S, likelihood_args=largs)
    assert _say("ref_cdf_" + lik, normwise(np.array(cdf), g[lik + "_cdf"])) < 1e-5
    ql, qu = _seeded(glm, glm.predict_interval, X[:12], 0.9, S, likelihood_args=tuple(a[:12] for a in largs))
    tol = 1e-4 if lik == "gaussian" else 1e-6
    _say("ref_interval_" + lik, max(_rel_q(ql, g[lik + "_ql"]), _rel_q(qu, g[lik + "_qu"])))
    assert np.all(np.abs(ql - g[lik + "_ql"]) < tol * np.maximum(1.0, np.abs(g[lik + "_ql"])))
    assert np.all(np.abs(qu - g[lik + "_qu"]) < tol * np.maximum(1.0, np.abs(g[lik + "_qu"])))


# ---- 2. against the host engine on the same latent samples ------------------------------------------------------------
def _step_margin(host, X, S, largs, tails):
    """Smallest distance of the host engine's sampled CDF, at any integer step inside the bracket and for any row, from the
    tail probabilities.  Below 0 the CDF is 0; the steps run up to where every row's sampled CDF has reached 1 - 1e-12 (from
    there on it stays within 1e-12 of 1)."""
    fs = _seeded(host, host._sample_matrix, X, S)
    N = X.shape[0]
    args = ([host.like_hypers_] if np.isscalar(host.like_hypers_) else list(host.like_hypers_)) \
        + [np.asarray(a, dtype=float).reshape(N, 1) for a in largs]
    margin, k = min(abs(0.0 - t) for t in tails), 0
    while True:
        c = host.likelihood.cdf(np.full((N, 1), float(k)), fs, *args).mean(axis=1)
        margin = min(margin, min(float(np.abs(c - t).min()) for t in tails))
        if c.min() >= 1.0 - 1e-12:
            return margin
        k += 1
        assert k < 5000, "the sampled CDF does not reach 1"


@pytest.mark.parametrize("S", [1, 50, 257])
@pytest.mark.parametrize("N", [1, 5, 259])
@pytest.mark.parametrize("lik", LIKS)
def test_device_engine_vs_host_engine(lik, N, S):
    """Both engines under the same seed: the same draws (and the same amount of the random stream consumed), the same
    float32 latent samples from the same GEMM, so what differs is libm and the order of the sums over the samples.  259 rows:
    a ragged last workgroup of 4 and more than 256 rows; 257 samples: more than one 256-column pad and more than the four
    values a lane keeps in registers; one sample: variance 0 and min = max = mean."""
    X, y, largs = _data(lik, N)
    host, dev = _model(lik, "host"), _model(lik, "device")

    Eh, Vh = _seeded(host, host.predict_moments, X, S, likelihood_args=largs)
    state_h = host.random_.get_state()
    Ed, Vd = _seeded(dev, dev.predict_moments, X, S, likelihood_args=largs)
    state_d = dev.random_.get_state()
    assert all(np.array_equal(a, b) for a, b in zip(state_h, state_d))
    tag = "_one_sample" if S == 1 else ""
    e_ey = _say("Ey" + tag, normwise(Ed, Eh))
    e_vy = _say("Vy" + tag, normwise(Vd, Vh))
    if S == 1:   # one sample: no spread, exactly
        assert not Vh.any() and not Vd.any()
    assert np.array_equal(_seeded(dev, dev.predict, X, S, likelihood_args=largs), Ed)

    lh = np.array(_seeded(host, host.predict_logpdf, X, y, S, likelihood_args=largs))
    ld = np.array(_seeded(dev, dev.predict_logpdf, X, y, S, likelihood_args=largs))
    e_lp = _say("logpdf" + tag, normwise(ld, lh))
    q = {"gaussian": 0.2, "bernoulli": 0.5, "binomial": 6.0, "poisson_exp": 2.0, "poisson_softplus": 1.0}[lik]
    ch = np.array(_seeded(host, host.predict_cdf, X, q, S, likelihood_args=largs))
    cd = np.array(_seeded(dev, dev.predict_cdf, X, q, S, likelihood_args=largs))
    e_cdf = _say("cdf" + tag, normwise(cd, ch))
    if S == 1:
        assert np.array_equal(ld[0], ld[1]) and np.array_equal(ld[0], ld[2])
        assert np.array_equal(cd[0], cd[1]) and np.array_equal(cd[0], cd[2])
    b_ey, b_vy, b_lp, b_cdf, b_q = BOUNDS_ONE_SAMPLE if S == 1 else BOUNDS
    assert e_ey < b_ey and e_vy <= b_vy and e_lp < b_lp and e_cdf < b_cdf

    qh = _seeded(host, host.predict_interval, X, 0.9, S, likelihood_args=largs)
    qd = _seeded(dev, dev.predict_interval, X, 0.9, S, likelihood_args=largs)
    assert not np.isnan(qh[0]).any() and not np.isnan(qh[1]).any()
    if lik == "gaussian":
        assert _say("gauss_interval" + tag, max(_rel_q(qd[0], qh[0]), _rel_q(qd[1], qh[1]))) < b_q
    else:
        # a step function: where the host's sampled CDF keeps its distance from the tails at EVERY step of EVERY row, no
        # rounding difference (test 3: below 1e-9) moves a quantile to another step, and the two bisections end on the same one
        assert _say("step_margin_" + lik, _step_margin(host, X, S, largs, (0.05, 0.95))) > STEP_MARGIN
        assert _say("count_interval" + tag, max(_rel_q(qd[0], qh[0]), _rel_q(qd[1], qh[1]))) <= 1e-9


def test_nan_intervals_have_the_host_engines_pattern():
    """NaN where the bracket [-reach, reach] does not straddle the tail probability.  Bernoulli: the sampled CDF is 0 at
    -reach and exactly 1 at reach whatever the row, so a percentile below 1 always has its bracket; one just ABOVE 1 puts
    the tails at -5e-10 and 1 + 5e-10, outside both ends, for every row.  Gaussian with a standard deviation of 1e4: the
    bracket of a row reaches 1000 max(mean f, 1), which contains the 5 % / 95 % quantiles only where f is above ~16.5 -- a
    mixed pattern over rows whose f runs from 0.5 to 39.5."""
    X, _, _ = _data("bernoulli", 7)
    host, dev = _model("bernoulli", "host"), _model("bernoulli", "device")
    qh = _seeded(host, host.predict_interval, X, 1.0 + 1e-9, 50)
    qd = _seeded(dev, dev.predict_interval, X, 1.0 + 1e-9, 50)
    assert np.isnan(qh[0]).all() and np.isnan(qh[1]).all()
    assert np.isnan(qd[0]).all() and np.isnan(qd[1]).all()

    host, dev = _model("gaussian", "host", scale=1e-3), _model("gaussian", "device", scale=1e-3)
    X = np.random.RandomState(2).randn(40, 3)
    X[:, 0] = np.arange(40) + 0.5
    for glm in (host, dev):
        glm.weights_[1, :] = 1.0   # f ~ X[:, 0]
        glm.like_hypers_ = 1e8
    qh = _seeded(host, host.predict_interval, X, 0.9, 50)
    qd = _seeded(dev, dev.predict_interval, X, 0.9, 50)
    for a, b in zip(qd, qh):
        assert 5 < np.isnan(b).sum() < 35
        assert np.array_equal(np.isnan(a), np.isnan(b))
        assert _say("gauss_interval_nan_case", _rel_q(a, b)) < BOUNDS[4]


# ---- 3. the special functions alone --------------------------------------------------------------------------------------
def _poisson_grid():
    mu, k = [], []
    for m in np.logspace(-8, 6, 13):
        ks = {0.0, 1.0, -1.0, 0.5, 1000.0 * m}
        for j in (0, 1, 3, 6, 10):
            ks.update(float(np.floor(m + sg * j * np.sqrt(m))) for sg in (-1, 1))
        for kk in sorted(ks):
            mu.append(m)
            k.append(kk)
    return np.array(mu), np.array(k)


def _binomial_grid():
    from scipy.special import expit
    n_, f_, k_ = [], [], []
    for n in (1, 7, 100, 10000):
        for f in (-30., -5., -0.3, 0., 2., 30.):
            p = expit(f)
            sd = np.sqrt(n * p * (1 - p))
            ks = {0.0, 1.0, -1.0, 0.5, float(n), float(n - 1), float(n + 1)}
            for j in (0, 1, 3, 6, 10):
                ks.update(float(np.clip(np.floor(n * p + sg * j * sd), -1, n + 1)) for sg in (-1, 1))
            for kk in sorted(ks):
                n_.append(float(n))
                f_.append(f)
                k_.append(kk)
    return np.array(n_), np.array(f_), np.array(k_)


def _rel(a, b):
    """largest relative difference over the finite entries; the non-finite ones must be the same"""
    a, b = np.asarray(a), np.asarray(b)
    fin = np.isfinite(b)
    assert np.array_equal(a[~fin], b[~fin]), (a[~fin], b[~fin])
    nz = fin & (b != 0)
    assert np.array_equal(a[fin & (b == 0)], b[fin & (b == 0)])
    return float((np.abs(a[nz] - b[nz]) / np.abs(b[nz])).max()) if nz.any() else 0.0


@pytest.fixture(scope="module")
def special_function_errors():
    """(largest absolute CDF error, largest relative loglike error, largest relative Ey error) of rr_lik_eval against the
    scipy calls of revrand_amd/likelihoods.py, per likelihood, on the grids described in test_device_likelihood_functions_vs_scipy -- evaluated once."""
    from revrand_amd import _hip, likelihoods as lk
    out = {}
    with np.errstate(all="ignore"):
        mu, k = _poisson_grid()
        for name, lid, f in (("poisson_exp", lk.RR_LIK_POISSON_EXP, np.log(mu)),
                             ("poisson_softplus", lk.RR_LIK_POISSON_SOFTPLUS, np.where(mu < 30, np.log(np.expm1(np.minimum(mu, 30))), mu))):
            like = _likelihood(name)
            out[name] = (np.abs(_hip.lik_eval("cdf", lid, f, k) - like.cdf(k, f)).max(),
                         _rel(_hip.lik_eval("loglike", lid, f, k), like.loglike(k, f)),
                         _rel(_hip.lik_eval("Ey", lid, f), like.Ey(f)))
        n, f, k = _binomial_grid()
        like = _likelihood("binomial")
        out["binomial"] = (np.abs(_hip.lik_eval("cdf", lk.RR_LIK_BINOMIAL, f, k, rowarg=n) - like.cdf(k, f, n)).max(),
                           _rel(_hip.lik_eval("loglike", lk.RR_LIK_BINOMIAL, f, k, rowarg=n), like.loglike(k, f, n)),
                           _rel(_hip.lik_eval("Ey", lk.RR_LIK_BINOMIAL, f, rowarg=n), like.Ey(f, n)))
        f = np.repeat([-30., -5., -0.3, 0., 2., 30.], 5)
        yb = np.tile([-1.0, 0.0, 0.5, 1.0, 2.0], 6)
        like = _likelihood("bernoulli")
        out["bernoulli"] = (np.abs(_hip.lik_eval("cdf", lk.RR_LIK_BERNOULLI, f, yb) - like.cdf(yb, f)).max(),
                            _rel(_hip.lik_eval("loglike", lk.RR_LIK_BERNOULLI, f, np.clip(yb, 0, 1) // 1), like.loglike(np.clip(yb, 0, 1) // 1, f)),
                            _rel(_hip.lik_eval("Ey", lk.RR_LIK_BERNOULLI, f), like.Ey(f)))
        var = 0.3
        z = np.linspace(-12, 12, 97)
        f = np.full_like(z, 0.7)
        yg = f + z * np.sqrt(var)
        like = _likelihood("gaussian")
        out["gaussian"] = (np.abs(_hip.lik_eval("cdf", lk.RR_LIK_GAUSSIAN, f, yg, lik_param=var) - like.cdf(yg, f, var)).max(),
                           _rel(_hip.lik_eval("loglike", lk.RR_LIK_GAUSSIAN, f, yg, lik_param=var), like.loglike(yg, f, var)),
                           _rel(_hip.lik_eval("Ey", lk.RR_LIK_GAUSSIAN, f, lik_param=var), like.Ey(f, var)))
    return out


@pytest.mark.parametrize("lik", LIKS)
def test_device_likelihood_functions_vs_scipy(special_function_errors, lik):
    """Poisson: mu at 13 log-spaced points from 1e-8 to 1e6, k in {0, 1, floor(mu +- j sqrt(mu)) for j = 0, 1, 3, 6, 10} and
    {-1, 0.5, 1000 mu}; binomial: n in {1, 7, 100, 10000}, p through f in {-30, -5, -0.3, 0, 2, 30}, the corresponding k and the
    ends of the support; Gaussian: (y - f) / sd in [-12, 12]; loglike and Ey at the same points."""
    e_cdf, e_ll, e_ey = special_function_errors[lik]
    _say("lik_eval_cdf_abs_" + lik, e_cdf)
    _say("lik_eval_loglike_rel_" + lik, e_ll)
    _say("lik_eval_Ey_rel_" + lik, e_ey)
    assert BOUND_CDF_ABS < 1e-9
    assert e_cdf < BOUND_CDF_ABS and e_ll < BOUND_LOGLIKE_REL and e_ey < BOUND_EY_REL


def test_lik_eval_refuses_bad_arguments():
    from revrand_amd import _hip, likelihoods as lk
    f = np.zeros(3)
    with pytest.raises(_hip.HipError):
        _hip.lik_eval("cdf", 9, f, f)                              # no such likelihood
    with pytest.raises(_hip.HipError):
        _hip.lik_eval("cdf", lk.RR_LIK_BINOMIAL, f, f)             # binomial without n
    with pytest.raises(_hip.HipError):
        _hip.lik_eval("cdf", lk.RR_LIK_GAUSSIAN, f, f, lik_param=0.0)   # variance
    with pytest.raises(_hip.HipError):
        _hip.lik_eval("loglike", lk.RR_LIK_POISSON_EXP, f)         # loglike without y
    with pytest.raises(ValueError):
        _hip.lik_eval("pdf", lk.RR_LIK_POISSON_EXP, f, f)


# ---- 4. chunking and sharding ---------------------------------------------------------------------------------------------
def test_row_chunks_equal_one_call_bit_for_bit():
    """N = 600 in chunks of 256 (256 + 256 + 88 rows) with a binomial n per row and targets per row: the per-row arguments must
    travel with their rows.  (F and S are small enough that the sample product of every chunk and of the one call runs on the
    small-product kernel, whose arithmetic per element does not depend on the row count.)"""
    from revrand_amd.basis_functions import MinibatchFeatures
    glm = _model("binomial", "device")
    X, y, (nbin,) = _data("binomial", 600)
    _, w = _seeded(glm, glm._draw_weights, X, 50)
    spec = glm.likelihood.predictive_spec([], [nbin], 600)
    feats = MinibatchFeatures(glm.basis)
    hyp = [glm.basis_hypers_]
    for what, kw in (("moments", {}), ("logpdf", {"y": y}), ("cdf", {"quantile": 6.0}), ("interval", {"p_lo": 0.05, "p_hi": 0.95})):
        one = feats.predictive(X, hyp, w, what, spec, **kw)
        parts = feats.predictive(X, hyp, w, what, spec, chunk_rows=256, **kw)
        assert one.shape == (600, 3 if what in ("logpdf", "cdf") else 2)
        assert np.array_equal(one, parts, equal_nan=True), what
        if what == "moments":   # and a chunk is not the whole: the rows differ from each other
            assert len(np.unique(one[:, 0])) > 500
    feats.release()


def test_row_shards_on_one_gpu_equal_one_context_bit_for_bit():
    X, _, largs = _data("binomial", 300)
    one = _model("binomial", "device")
    two = _model("binomial", "device", devices=[0, 0])
    for name, args in (("predict_moments", (X, 50)), ("predict_interval", (X, 0.9, 50))):
        a = _seeded(one, getattr(one, name), *args, likelihood_args=largs)
        b = _seeded(two, getattr(two, name), *args, likelihood_args=largs)
        for u, v in zip(a, b):
            assert u.shape == (300,) and np.array_equal(u, v, equal_nan=True), name


def test_predictive_refuses_bad_arguments():
    from revrand_amd import _hip, likelihoods as lk
    fm = _hip.FeatureMatrix(8, 4)
    fm.begin(8)
    fm.put_host(np.ones((8, 4)), 0)
    W = np.ones((4, 3))
    with pytest.raises(_hip.HipError):
        fm.predictive(8, W, "moments", 9)                                   # no such likelihood
    with pytest.raises(_hip.HipError):
        fm.predictive(8, W, "moments", lk.RR_LIK_BINOMIAL)                  # binomial without n
    with pytest.raises(_hip.HipError):
        fm.predictive(8, W, "moments", lk.RR_LIK_GAUSSIAN, 0.0)             # variance
    with pytest.raises(ValueError):
        fm.predictive(8, W, "logpdf", lk.RR_LIK_POISSON_EXP)                # no targets
    with pytest.raises(ValueError):
        fm.predictive(8, W, "median", lk.RR_LIK_POISSON_EXP)
    with pytest.raises(ValueError):
        fm.predictive(8, np.ones((5, 3)), "moments", lk.RR_LIK_POISSON_EXP)  # W is not (F, S)
    out = fm.predictive(8, W, "moments", lk.RR_LIK_POISSON_EXP)             # (and the handle still works)
    assert out.shape == (8, 2) and np.allclose(out[:, 0], np.exp(4.0)) and np.allclose(out[:, 1], 0.0, atol=1e-20)
