"""rr_glm_sviw / GeneralizedLinearModel(wide_fused=True): the small-minibatch SVI loop for bases too wide for the LDS kernel of
rr_svi.hip -- a fixed chain of four kernels per step, many steps queued per library call (rr_svi_wide.hip) -- against

1. the fits THE REFERENCE computed (tests/golden/glm_fit.npz), forced onto the wide loop with four frequencies per item, so
   that every Fourier child spans two items and the linear child a third;
2. the float64 oracle (oracle/revrand_oracle.py: glm_fit, pinned to the reference by tests/test_oracle_golden.py) at F = 1356;
3. the step-per-call loop and the host loop on the same minibatches and draws at F = 900 (minibatch x F = 9000: outside the LDS
   kernel's range), every likelihood, every updater, isotropic / bounded / apply_ind bases;
4. the step-per-call loop under the device sampler;
5. itself: two runs, every cut into blocks of steps and every cut of the random starts into chunks give the same bits;
6. the sequential evaluation of the random starts;
7. the edges of its range and of the item split;
8. the routing: who takes which loop.

Every fit asserts which loop ran (spies on WideSvi.run / .starts, FusedSvi.run, ResidentSgd.step) and that the estimator's
RandomState ends where the comparison's does."""
import functools

import numpy as np
import pytest

from conftest import normwise
from glm_fit_cases import IMPLEMENTED

pytestmark = pytest.mark.gpu

KERNELS = ("rr_glm_sviw_a_kernel", "rr_glm_sviw_b_kernel", "rr_glm_sviw_c_kernel", "rr_glm_sviw_d_kernel")


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd import optimize as opt
    from revrand_amd.btypes import Bound, Parameter, Positive
    from revrand_amd.glm import GeneralizedLinearModel
    return bs, lk, opt, Bound, Parameter, Positive, GeneralizedLinearModel


class _Spies(object):
    """counts what each loop ran while a fit is inside `with`"""

    def __init__(self, record=None):
        self.calls = {"wide": 0, "wide_runs": 0, "wide_starts": 0, "start_calls": 0, "fused": 0, "resident": 0}
        self.record = record

    def __enter__(self):
        from revrand_amd import _hip
        self._hip = _hip
        self.real = (_hip.WideSvi.run, _hip.WideSvi.starts, _hip.FusedSvi.run, _hip.ResidentSgd.step)
        real_wrun, real_wstarts, real_frun, real_step = self.real
        self.real_read = _hip.FusedSvi.read
        real_read = self.real_read

        def read(self):
            out = real_read(self)
            if isinstance(self, _hip.WideSvi):
                calls["read"] = tuple(np.array(v) for v in out)
            return out
        _hip.FusedSvi.read = read
        calls, record = self.calls, self.record

        def wrun(self, n, *a, **k):
            calls["wide"] += n
            calls["wide_runs"] += 1
            return real_wrun(self, n, *a, **k)

        def wstarts(self, didx, cand, *a, **k):
            calls["wide_starts"] += len(cand)
            calls["start_calls"] += 1
            out = real_wstarts(self, didx, cand, *a, **k)
            if record is not None:
                record.append(np.array(out))
            return out

        def frun(self, n, *a, **k):
            calls["fused"] += n
            return real_frun(self, n, *a, **k)

        def step(self, *a, **k):
            calls["resident"] += 1
            return real_step(self, *a, **k)
        _hip.WideSvi.run, _hip.WideSvi.starts, _hip.FusedSvi.run, _hip.ResidentSgd.step = wrun, wstarts, frun, step
        return self.calls

    def __exit__(self, *exc):
        h = self._hip
        h.WideSvi.run, h.WideSvi.starts, h.FusedSvi.run, h.ResidentSgd.step = self.real
        h.FusedSvi.read = self.real_read
        return False


def _flat(v):
    v = v if isinstance(v, (list, tuple)) else [v]
    return np.concatenate([np.ravel(np.asarray(u, dtype=float)) for u in v] + [np.empty(0)])


def _result(glm):
    return (glm.weights_.copy(), glm.covariance_.copy(), _flat(glm.regularizer_), _flat(glm.like_hypers_), _flat(glm.basis_hypers_),
            glm.random_.randn())


def _worst(a, b):
    errs = []
    for u, v in zip(a[:5], b[:5]):
        assert u.shape == v.shape
        errs.append(normwise(u, v) if u.size else 0.0)
    return max(errs)


def _same(a, b, tol):
    w = _worst(a, b)
    assert w < tol, (w, tol)
    assert a[5] == b[5]      # the stream ends where the comparison's does


# ---- the shape of tests 3 - 6: RandomRBF(450, ARD, Xdim = 4), M = 10: minibatch x F = 9000 ------------------------------------
def _data(lik, N=500, d=4, seed=4):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, d)
    f = 0.5 * np.sin(X[:, 0]) + 0.2 * X[:, 2]
    if lik in ("poisson", "poisson_softplus"):
        return X, rs.poisson(np.exp(f)).astype(float), ()
    if lik == "bernoulli":
        return X, (rs.rand(N) < 1 / (1 + np.exp(-3 * f))).astype(float), ()
    if lik == "binomial":
        n = rs.randint(5, 30, size=N).astype(float)
        return X, rs.binomial(n.astype(int), 1 / (1 + np.exp(-3 * f))).astype(float), (n,)
    return X, f + 0.1 * rs.randn(N), ()


def _basis(kind, d, n=450):
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    if kind == "ard":
        return bs.RandomRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
    if kind == "iso":
        return bs.RandomRBF(nbases=n, Xdim=d, random_state=1)
    if kind == "bound":
        return bs.RandomRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(1.0, Bound(0.995, 1.004)))
    if kind == "posupper":
        return bs.RandomRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(1.0, Positive(1.03)))
    if kind == "cat_ind":   # children on their own columns of X, a linear child without the column of ones
        return bs.RandomRBF(nbases=n, Xdim=2, random_state=1, apply_ind=[0, 2]) + bs.LinearBasis(onescol=False, apply_ind=[1, 3])
    if kind == "one":       # a Fourier child with ONE frequency next to a wider one
        return bs.RandomRBF(nbases=1, Xdim=d, random_state=1) + bs.RandomMatern52(nbases=20, Xdim=d, random_state=2)
    if kind == "item+1":    # one frequency more than an item of the default width holds
        return bs.RandomRBF(nbases=65, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
    if kind == "boundary":  # a child ends in the middle of the default item width; the next starts an item of its own
        return bs.RandomRBF(nbases=32, Xdim=d, random_state=1) + bs.LinearBasis(onescol=True) \
            + bs.RandomMatern52(nbases=100, Xdim=d, random_state=2, lenscale=Parameter(np.ones(d), Positive()))
    raise ValueError(kind)


UPDATERS = {"SGDUpdater": lambda opt: opt.SGDUpdater(eta=1e-4), "Momentum": lambda opt: opt.Momentum(rho=0.5, eta=1e-4),
            "AdaGrad": lambda opt: opt.AdaGrad(eta=1e-2), "AdaDelta": lambda opt: opt.AdaDelta(), "Adam": lambda opt: opt.Adam()}


def _fit(loop, lik="poisson", updater=None, basis="ard", sampler="host", maxiter=25, K=4, L=10, batch=10, nstarts=3, block=None,
         block_bytes=None, record=None, n=450, N=500, force=False, wide_fused=None, devices=None):
    """loop: "wide" (wide_fused=True), "resident" (the step-per-call loop), "host" (optimize.sgd around `_elbo`)"""
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    from revrand_amd import glm as glm_mod
    X, y, largs = _data(lik, N=N)
    like = {"poisson": lambda: lk.Poisson(), "poisson_softplus": lambda: lk.Poisson("softplus"), "bernoulli": lk.Bernoulli,
            "binomial": lk.Binomial, "gaussian": lk.Gaussian}[lik]()
    glm = GLM(like, _basis(basis, X.shape[1], n), K=K, nsamples=L, batch_size=batch, maxiter=maxiter, nstarts=nstarts, random_state=11,
              updater=UPDATERS[updater](opt) if updater is not None else None, sampler=sampler,
              wide_fused=(loop == "wide") if wide_fused is None else wide_fused, devices=devices)
    glm._resident_sgd = loop != "host"
    glm._wide_fused_force = force
    saved = (glm_mod._FusedLoop.BLOCK_STEPS, glm_mod._FusedLoop.BLOCK_BYTES)
    if block is not None:
        glm_mod._FusedLoop.BLOCK_STEPS = block
    if block_bytes is not None:
        glm_mod._FusedLoop.BLOCK_BYTES = block_bytes
    try:
        with _Spies(record) as calls:
            np.random.seed(3)
            glm.fit(X, y, likelihood_args=largs)
    finally:
        glm_mod._FusedLoop.BLOCK_STEPS, glm_mod._FusedLoop.BLOCK_BYTES = saved
    return _result(glm), dict(calls)


def _ran_wide(calls, steps, starts):
    assert calls["wide"] == steps and calls["wide_starts"] == starts and calls["fused"] == 0 and calls["resident"] == 0, calls


@functools.lru_cache(maxsize=None)
def _reference_fit(loop, lik="poisson", updater=None, basis="ard", sampler="host", **kw):
    """a comparison fit (host or step-per-call loop), made once and shared; it counts its own steps"""
    out, calls = _fit(loop, lik, updater=updater, basis=basis, sampler=sampler, **dict(kw))
    assert calls["wide"] == 0 and calls["fused"] == 0
    assert calls["resident"] == (dict(kw).get("maxiter", 25) if loop == "resident" else 0)
    return out


# ---- 1. the reference's own fits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IMPLEMENTED, ids=[c[0] for c in IMPLEMENTED])
def test_reference_fits_on_the_wide_loop(golden, case, monkeypatch):
    """All implemented cases of glm_fit.npz, RR_SVIW_ITEM=4 (8 frequencies per child: two items each, the linear child a third),
    at the project's bound for a fit on any loop: 1e-4 normwise per block (tests/test_gpu_glm_fit.py)."""
    from test_gpu_glm_fit import TOL, _model
    assert TOL == 1e-4
    monkeypatch.setenv("RR_SVIW_ITEM", "4")
    g = golden("glm_fit")
    tag, lik = case[0], case[1]
    glm, largs = _model(g, case)
    glm.wide_fused = True
    glm._wide_fused_force = True
    with _Spies() as calls:
        np.random.seed(int(g["global_seed"]))
        glm.fit(g["X"], g["y_" + ("poisson_exp" if lik == "poisson_softplus" else lik)], likelihood_args=largs)
    _ran_wide(calls, int(g["maxiter"]), case[4])     # the random-start count and the loop that ran
    errs = {"m": normwise(glm.weights_, g[tag + "_m"]), "C": normwise(glm.covariance_, g[tag + "_C"]),
            "reg": normwise(_flat(glm.regularizer_), g[tag + "_reg"]), "ls": normwise(_flat(glm.basis_hypers_), g[tag + "_ls"])}
    if lik == "gaussian":
        errs["lik"] = normwise(_flat(glm.like_hypers_), g[tag + "_lik"])
    worst = max(errs, key=errs.get)
    print("%s: worst block %s %.3e" % (tag, worst, errs[worst]))
    assert errs[worst] < TOL, errs
    assert glm.random_.randn() == float(g[tag + "_end"])


# ---- 2. wide shapes against the oracle ----------------------------------------------------------------------------------------
# Asserted at 1e-4 first (the project's bound for a fit on any loop); measured on an MI355X: worst block 3.5e-9 (Gaussian, C) and
# 1.7e-8 (Poisson, C) -- where the LDS kernel stands on the golden cases (5e-8).  The bound is 10 x the recorded worst.
ORACLE_TOL = 1.7e-7


@pytest.mark.parametrize("lik", ["gaussian", "poisson"])
def test_wide_shape_against_the_oracle(lik):
    """N = 300, d = 5; LinearBasis(onescol) + RandomRBF(600, ARD) + RandomMatern52(75, isotropic): F = 1356, outside the LDS
    kernel's range at 10 rows without forcing.  K = 3, L = 6, 20 Adam steps, 2 starts, the reference's stream.  (X holds float32
    values: the resident rows are float32, and the comparison is of the loop, not of the input's rounding.)"""
    import revrand_oracle as orc
    from scipy.stats import gamma
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    rs = np.random.RandomState(21)
    N, d = 300, 5
    X = rs.randn(N, d).astype(np.float32).astype(float)
    f = 0.5 * np.sin(X[:, 0]) + 0.2 * X[:, 2]
    y = f + 0.1 * rs.randn(N) if lik == "gaussian" else rs.poisson(np.exp(f)).astype(float)
    basis = bs.LinearBasis(onescol=True) \
        + bs.RandomRBF(nbases=600, Xdim=d, random_state=3, lenscale=Parameter(gamma(4., scale=0.25), Positive(), shape=(d,))) \
        + bs.RandomMatern52(nbases=75, Xdim=d, random_state=4)
    glm = GLM(lk.Gaussian() if lik == "gaussian" else lk.Poisson(), basis, K=3, nsamples=6, batch_size=10, maxiter=20, nstarts=2,
              random_state=7, wide_fused=True)
    assert glm._wide_fused_force is False
    with _Spies() as calls:
        np.random.seed(5)
        glm.fit(X, y)
    _ran_wide(calls, 20, 2)
    assert glm.weights_.shape == (1356, 3)
    P = orc.ParamSpec
    reg = lambda: P(dist=gamma(1.), positive=True)  # noqa: E731
    o = orc.glm_fit(X, y, "gaussian" if lik == "gaussian" else "poisson_exp", [],
                    [("linear", True), ("rff", basis.bases[1].W, d), ("rff", basis.bases[2].W, 1)], [reg(), reg(), reg()],
                    [P(dist=gamma(1.), positive=True)] if lik == "gaussian" else [],
                    [P(value=[]), P(dist=gamma(4., scale=0.25), positive=True, shape=(d,)), P(dist=gamma(1.), positive=True)],
                    3, 6, 10, 20, 2, 7, 5, sgd_batch_size=10)
    want = (o[0], o[1], _flat(list(o[2])), _flat(list(o[3])), _flat(list(o[4])), o[7])
    got = _result(glm)
    names = ("m", "C", "reg", "lik", "ls")
    errs = {nm: (normwise(u, v) if u.size else 0.0) for nm, u, v in zip(names, got[:5], want[:5])}
    worst = max(errs, key=errs.get)
    print("oracle, %s: worst block %s %.3e" % (lik, worst, errs[worst]))
    assert errs[worst] < ORACLE_TOL, errs
    assert got[5] == want[5]


# ---- 3. wide == step-per-call loop == host loop ---------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", ["poisson", "poisson_softplus", "bernoulli", "binomial", "gaussian"])
def test_wide_loop_equals_the_other_two(lik):
    wide, calls = _fit("wide", lik)
    _ran_wide(calls, 25, 3)
    _same(wide, _reference_fit("host", lik), 2e-5)
    _same(wide, _reference_fit("resident", lik), 2e-5)


@pytest.mark.parametrize("name", ["SGDUpdater", "AdaDelta", "AdaGrad", "Momentum", "Adam"])
def test_every_updater(name):
    wide, calls = _fit("wide", "poisson", updater=name)
    _ran_wide(calls, 25, 3)
    _same(wide, _reference_fit("host", "poisson", updater=name), 2e-5)


@pytest.mark.parametrize("basis", ["iso", "bound", "cat_ind"])
def test_bases_and_bounds(basis):
    for lik in ("gaussian", "poisson"):
        wide, calls = _fit("wide", lik, basis=basis)
        _ran_wide(calls, 25, 3)
        _same(wide, _reference_fit("host", lik, basis=basis), 2e-5)


# ---- 4. the device sampler -----------------------------------------------------------------------------------------------------
def test_device_sampler_equals_the_step_per_call_loop():
    for lik in ("poisson", "gaussian"):
        wide, calls = _fit("wide", lik, sampler="device")
        _ran_wide(calls, 25, 3)
        _same(wide, _reference_fit("resident", lik, sampler="device"), 2e-5)


# ---- 5. bitwise -----------------------------------------------------------------------------------------------------------------
def _bits(a, b):
    for u, v in zip(a[:5], b[:5]):
        assert np.array_equal(u, v)
    assert a[5] == b[5]


def test_runs_and_blocks_of_steps_are_bit_identical():
    outs = {}
    for sampler in ("device", "host"):
        first, c = _fit("wide", "gaussian", sampler=sampler)
        again, _ = _fit("wide", "gaussian", sampler=sampler)
        _ran_wide(c, 25, 3)
        _bits(first, again)
        z, objs, norms = c["read"]
        assert objs.shape == norms.shape == (25,) and np.all(np.isfinite(objs)) and np.all(norms > 0)
        for block, runs in ((1, 25), (7, 4), (256, 1)):
            cut, cc = _fit("wide", "gaussian", sampler=sampler, block=block)
            assert cc["wide_runs"] == runs and cc["wide"] == 25
            _bits(first, cut)
            for u, v in zip(c["read"], cc["read"]):     # z, objectives and norms as the object hands them back
                assert np.array_equal(u, v)
        outs[sampler] = first


def test_chunked_random_starts_are_bit_identical():
    """BLOCK_BYTES lowered so that 5 candidates take 3 chunks: the same objectives, winner, fit and stream end"""
    K, L, F = 4, 10, 900
    per = (2 * F * K + 1 + 1 + 4) * 8 + K * L * F * 4
    rec1, rec2 = [], []
    whole, c1 = _fit("wide", "gaussian", nstarts=5, maxiter=5, record=rec1)
    cut, c2 = _fit("wide", "gaussian", nstarts=5, maxiter=5, record=rec2, block_bytes=2 * per + 16)
    assert c1["start_calls"] == 1 and c2["start_calls"] >= 3 and c1["wide_starts"] == c2["wide_starts"] == 5
    a, b = np.concatenate(rec1), np.concatenate(rec2)
    assert np.array_equal(a, b) and int(np.argmin(a)) == int(np.argmin(b))
    _bits(whole, cut)


# ---- 6. batched starts == sequential evaluation ----------------------------------------------------------------------------------
def test_batched_random_starts_score_like_the_sequential_evaluation():
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    rec = []
    wide, calls = _fit("wide", "gaussian", nstarts=12, maxiter=2, record=rec)
    _ran_wide(calls, 2, 12)
    seq = []
    real = GLM._elbo

    def spy(self, *a, objective_only=False, **k):
        out = real(self, *a, objective_only=objective_only, **k)
        if objective_only:
            seq.append(out)
        return out
    GLM._elbo = spy
    try:
        host, _ = _fit("host", "gaussian", nstarts=12, maxiter=2)
    finally:
        GLM._elbo = real
    got = np.concatenate(rec)
    assert len(seq) == 12 and got.shape == (12,)
    assert normwise(got, np.array(seq)) < 1e-6
    assert int(np.argmin(got)) == int(np.argmin(seq))
    _same(wide, host, 2e-5)


# ---- 7. edges -------------------------------------------------------------------------------------------------------------------
EDGES = {"K1_L5_M7": dict(K=1, L=5, batch=7, n=40), "K32_L3_M64": dict(K=32, L=3, batch=64, n=40),
         "K8_L20_M16": dict(K=8, L=20, batch=16, n=40), "one_frequency": dict(basis="one"), "item_plus_one": dict(basis="item+1"),
         "child_boundary": dict(basis="boundary"), "one_minibatch_of_all_rows": dict(N=40, batch=40, n=40),
         "bound_run_into": dict(basis="bound", n=40), "positive_upper": dict(basis="posupper", n=40)}


@pytest.mark.parametrize("edge", sorted(EDGES))
def test_edges_against_the_host_loop(edge):
    kw = dict(EDGES[edge])
    wide, calls = _fit("wide", "poisson", maxiter=20, nstarts=2, force=True, **kw)
    _ran_wide(calls, 20, 2)
    host, c = _fit("host", "poisson", maxiter=20, nstarts=2, **kw)
    assert c["wide"] == c["fused"] == c["resident"] == 0
    _same(wide, host, 2e-5)
    if edge == "positive_upper":
        assert float(wide[4][0]) <= 1.03 * (1 + 1e-12)
    if edge == "bound_run_into":
        assert 0.995 <= float(wide[4][0]) <= 1.004


# ---- 8. routing -------------------------------------------------------------------------------------------------------------------
def test_default_keeps_the_step_per_call_loop_at_wide_shapes():
    out, calls = _fit("resident", "poisson", maxiter=6, wide_fused=False)     # F = 900
    assert calls["resident"] == 6 and calls["wide"] == 0 and calls["fused"] == 0 and calls["wide_starts"] == 0


def test_shapes_of_the_lds_kernel_still_take_it():
    out, calls = _fit("wide", "poisson", maxiter=6, n=12)     # the golden shapes' size: F = 24
    assert calls["fused"] == 6 and calls["wide"] == 0 and calls["resident"] == 0 and calls["wide_starts"] == 0


def test_other_children_keep_the_step_per_call_loop():
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    X, y, _ = _data("poisson")
    basis = bs.RadialBasis(centres=X[:30].copy(), lenscale=Parameter(np.ones(4), Positive())) \
        + bs.RandomRBF(nbases=450, Xdim=4, random_state=1)
    glm = GLM(lk.Poisson(), basis, K=4, nsamples=10, batch_size=10, maxiter=6, nstarts=2, random_state=11, resident_bases="all",
              wide_fused=True)
    with _Spies() as calls:
        np.random.seed(3)
        glm.fit(X, y)
    assert calls["resident"] == 6 and calls["wide"] == 0 and calls["fused"] == 0 and calls["wide_starts"] == 0


def test_device_group_with_small_minibatches_takes_the_wide_loop_on_member_0():
    one, c1 = _fit("wide", "poisson", maxiter=10)
    many, c2 = _fit("wide", "poisson", maxiter=10, devices=[0, 0])
    _ran_wide(c1, 10, 3)
    _ran_wide(c2, 10, 3)
    _bits(one, many)


# ---- the launches of a step (the bounds-checking build counts them: tests/test_gpu_fused_wide_debug.py) ---------------------------
def test_launches_per_step_and_per_candidate():
    """n steps are n x (A, B, C, D), n candidates n x (A, B, D): counted by rr_debug_kernel_launches in the bounds-checking
    build; the release build counts nothing (-1)."""
    from revrand_amd import _hip
    lib = _hip.load_library()
    debug = bool(lib.rr_build_flags() & 1)
    lib.rr_debug_kernel_launches(None)
    out, calls = _fit("wide", "poisson", maxiter=9, nstarts=4, block=4)
    _ran_wide(calls, 9, 4)
    counts = [lib.rr_debug_kernel_launches(k.encode()) for k in KERNELS]
    if debug:
        assert counts == [9 + 4, 9 + 4, 9, 9 + 4], counts
        assert lib.rr_debug_kernel_launches(b"rr_glm_sviw_x_kernel") == 2     # create, set_start: not part of a step
        assert lib.rr_debug_kernel_launches(b"rr_glm_svi_steps_kernel") == 0
    else:
        assert counts == [-1] * 4
