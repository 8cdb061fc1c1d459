"""Row e' of the round-4 verdict: several GPUs behind the UNCHANGED single-process estimator call --
``StandardLinearModel(basis, devices=[...]).fit(X, y)`` / ``basis.gram(X, y, l, devices=[...])`` (revrand_amd/multigpu.py,
``rr_comm_init_all`` / ``rr_comm_group_*`` in include/revrand_hip.h).  The reference's fit is one call in one process
(revrand/slm.py:74-140) driven by sklearn Pipelines / GridSearchCV (tests/test_models.py:39-80).

The test box has ONE GPU: the members of every group here share it (``devices=[0, 0]``, ``[0, 0, 0, 0]``) and take the
library's peer transport -- the same kernels that load a peer's HBM over xGMI when the members have a GPU each.  What is
checked: the in-process collective itself against NumPy (sum / max / min, ragged counts, broadcast), the sharded statistics,
`_elbo`, `fit` and `predict_moments` against the one-context results, bitwise agreement of the members and run-to-run
reproducibility in deterministic mode, sklearn's clone / pickle / GridSearchCV on an estimator with ``devices=``."""
import pickle

import numpy as np
import pytest

import revrand_oracle as orc
from conftest import normwise

pytestmark = pytest.mark.gpu


def _setup():
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip, multigpu
    from revrand_amd.btypes import Parameter, Positive
    from revrand_amd.slm import StandardLinearModel
    return bs, _hip, multigpu, Parameter, Positive, StandardLinearModel


def _data(N, d, seed=0):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, d).astype(np.float32)
    y = (np.sin(X @ rs.randn(d)) + 0.1 * rs.randn(N)).astype(np.float32)
    return X, y


@pytest.mark.parametrize("n", [1, 2, 4, 7])
def test_group_allreduce_and_broadcast_vs_numpy(n):
    """rr_comm_group_allreduce_dev / _broadcast_dev on members sharing the GPU: every op, counts that do not divide into
    slices (1, 31, 33, a prime, 1 << 20 + 3), every member bit-identical to NumPy's sum in member order."""
    bs, _hip, multigpu, *_ = _setup()
    g = multigpu.DeviceGroup([0] * n, transport="peer")
    try:
        assert g.transport == "peer" and g.n == n
        rs = np.random.RandomState(n)
        for count in (1, 31, 33, 4099, (1 << 20) + 3):
            host = [rs.randn(count) * 10.0 ** rs.randint(-3, 4) for _ in range(n)]
            for op, ref in (("sum", None), ("max", np.maximum), ("min", np.minimum)):
                bufs = [m.upload_vector(h) for m, h in zip(g.members, host)]
                g.allreduce_device(bufs, count, op)
                if ref is None:
                    want = host[0].copy()
                    for h in host[1:]:
                        want = want + h       # the transport's order: member 0, 1, ...
                else:
                    want = host[0]
                    for h in host[1:]:
                        want = ref(want, h)
                for m, b in zip(g.members, bufs):
                    got = m.download(b, (count,), np.float64)
                    assert np.array_equal(got, want), (n, count, op)
                    b.free()
        count = 70001
        host = [rs.randn(count) for _ in range(n)]
        for root in sorted({0, n - 1}):
            bufs = [m.upload_vector(h) for m, h in zip(g.members, host)]
            g.broadcast_device(bufs, count * 8, root)
            for m, b in zip(g.members, bufs):
                assert np.array_equal(m.download(b, (count,), np.float64), host[root])
                b.free()
    finally:
        g.close()


def test_group_rejects_what_it_cannot_do():
    bs, _hip, multigpu, *_ = _setup()
    with pytest.raises(_hip.HipError, match="one member per device"):
        multigpu.DeviceGroup([0, 0], transport="rccl")
    with pytest.raises(ValueError):
        multigpu.resolve_devices([])
    g = multigpu.DeviceGroup([0, 0], transport="peer")
    try:
        buf = g.members[0].upload_vector(np.ones(8))
        # the per-rank collective on a member of an in-process group would wait for its peers forever: refused
        rc = g.lib.rr_comm_allreduce_dev(g._comms[0], buf.ptr, 8, 0)
        assert rc == -5 and b"rr_comm_group_allreduce_dev" in g.lib.rr_last_error()
        with pytest.raises(_hip.HipError, match="share a buffer"):
            g.allreduce_device([buf, buf], 8)
        buf.free()
    finally:
        g.close()


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]])
def test_sharded_statistics_equal_the_one_context_statistics(devices):
    """basis.gram(X, y, l, devices=...) against the same call on one context and against the oracle; a ragged row count
    (shards differ by a row), F = 2 x 300 (ragged SYRK tiles)."""
    bs, _hip, multigpu, Parameter, Positive, SLM = _setup()
    N, d, n = 100_003, 8, 300
    X, y = _data(N, d)
    ls = np.linspace(0.8, 1.3, d)
    basis = bs.RandomRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
    G1, b1, t1 = basis.gram(X, y, ls)
    G, b, t = basis.gram(X, y, ls, devices=devices)
    assert np.array_equal(G, G.T)
    # (not bitwise: the SYRK accumulates in f32 inside a K-split of rows and in f64 across them, and sharding regroups rows)
    assert normwise(G, G1) < 2e-6 and normwise(b, b1) < 2e-6 and abs(t - t1) < 1e-12 * t1
    sl = slice(0, 4096)
    Gr, br, _ = orc.gram_stats(orc.rff_transform(X[sl], basis.W, ls), y[sl].astype(np.float64))
    Gs, bsub, _ = basis.gram(X[sl], y[sl], ls, devices=devices)
    assert normwise(Gs, Gr) < 1e-3 and normwise(bsub, br) < 1e-3
    # concatenation of config 3's form: Matern52 + Linear through the resident feature matrix of every member
    cat = bs.RandomMatern52(nbases=256, Xdim=d, random_state=2, lenscale=Parameter(np.ones(d), Positive())) + bs.LinearBasis(onescol=True)
    Gc1, bc1, tc1 = cat.gram(X, y, ls)
    Gc, bc, tc = cat.gram(X, y, ls, devices=devices)
    assert normwise(Gc, Gc1) < 2e-6 and normwise(bc, bc1) < 2e-6 and abs(tc - tc1) < 1e-12 * tc1


def _elbo_once(SLM, basis, X, y, var, reg, ls, devices=None, keep_state=False):
    slm = SLM(basis, devices=devices)
    slm.obj_ = -np.inf
    slm._state = slm._make_state(X, y)
    assert slm._state is not None
    f, (gv, gr, gh) = slm._elbo(X, y, var, reg, ls)
    C = slm._state.best_covariance() if getattr(slm._state, "best_on_device", False) else slm.covariance_
    extra = None
    if keep_state:  # every member's copy of the statistics and of the covariance, for the bitwise checks
        st = slm._state
        extra = ([s.stats_host() for s in st.states],
                 [s.dev.download(s.dCbest, (s.F, s.F), np.float64) for s in st.states])
    slm._state.release()
    slm._state = None
    from revrand_amd.utils import flatten_values
    flat = np.asarray(flatten_values([f, gv, gr, gh]), dtype=float)
    return flat, slm.weights_, np.array(C), extra


@pytest.mark.parametrize("devices", [[0, 0], [0, 0, 0, 0]])
def test_sharded_elbo_equals_the_one_context_elbo(devices):
    """One `_elbo` (objective, dvar, dreg, dhyp, weights, covariance) with the rows on 2 / 4 members against one context,
    single basis (ARD and the isotropic dimension-0 gradient) and a concatenation; posterior on the device."""
    bs, _hip, multigpu, Parameter, Positive, SLM = _setup()
    import os
    os.environ["RR_POSDEF"] = "device"
    try:
        N, d, n = 60_001, 6, 192
        X, y = _data(N, d, seed=3)
        ls = np.linspace(0.7, 1.4, d)
        ard = bs.RandomRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
        iso = bs.RandomRBF(nbases=n, Xdim=d, random_state=1)
        cat = bs.RandomMatern52(nbases=128, Xdim=d, random_state=2, lenscale=Parameter(np.ones(d), Positive())) \
            + bs.LinearBasis(onescol=True)
        for basis, reg, hyp in ((ard, 1.2, ls), (iso, 1.2, 0.9), (cat, [1.2, 0.8], ls)):
            v1, w1, C1, _ = _elbo_once(SLM, basis, X, y, 0.3, reg, hyp)
            v, w, C, _ = _elbo_once(SLM, basis, X, y, 0.3, reg, hyp, devices=devices)
            assert v.shape == v1.shape
            assert abs(v[0] - v1[0]) < 1e-6 * abs(v1[0]) and normwise(v[1:], v1[1:]) < 1e-4, (v, v1)   # f32 row sums regrouped
            assert normwise(w, w1) < 2e-4 and normwise(C, C1) < 2e-4   # (conditioning amplifies the regrouped f32 sums)
    finally:
        os.environ.pop("RR_POSDEF", None)


def test_members_agree_bitwise_and_runs_reproduce_in_deterministic_mode():
    bs, _hip, multigpu, Parameter, Positive, SLM = _setup()
    import os
    os.environ["RR_POSDEF"] = "device"
    devices = [0, 0, 0]
    g = multigpu.get_group(devices)
    prev = g.set_deterministic(True)
    try:
        N, d, n = 90_002, 8, 300
        X, y = _data(N, d, seed=5)
        ls = np.linspace(0.8, 1.3, d)
        basis = bs.RandomRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
        runs = [_elbo_once(SLM, basis, X, y, 0.3, 1.2, ls, devices=devices, keep_state=True) for _ in range(2)]
        for (stats, covs) in (r[3] for r in runs):
            for (G, b, t), C in zip(stats[1:], covs[1:]):     # every member: the same statistics, the same posterior
                assert np.array_equal(G, stats[0][0]) and np.array_equal(b, stats[0][1]) and t == stats[0][2]
                assert np.array_equal(C, covs[0])
        a, bb = runs
        assert np.array_equal(a[0], bb[0]) and np.array_equal(a[1], bb[1]) and np.array_equal(a[2], bb[2])
    finally:
        for m, p in zip(g.members, prev):
            m.set_deterministic(p)
        os.environ.pop("RR_POSDEF", None)


def test_fit_and_predict_with_devices_equal_the_one_context_fit():
    """`fit` end to end (L-BFGS-B on the sharded `_elbo`) and `predict` / `predict_moments` on sharded query rows."""
    bs, _hip, multigpu, Parameter, Positive, SLM = _setup()
    N, d, n = 20_000, 5, 160
    X, y = _data(N, d, seed=7)
    Xq, _ = _data(70_001, d, seed=8)

    def make(devices):
        basis = bs.RandomRBF(nbases=n, Xdim=d, random_state=4, lenscale=Parameter(np.ones(d), Positive()))
        return SLM(basis, nstarts=0, maxiter=25, random_state=0, devices=devices)
    one = make(None).fit(X, y)
    two = make([0, 0]).fit(X, y)
    assert abs(two.obj_ - one.obj_) < 1e-5 * abs(one.obj_)
    assert normwise(two.weights_, one.weights_) < 2e-3 and abs(two.var_ - one.var_) < 1e-3 * one.var_
    Ey1, Vy1 = two.predict_moments(Xq)
    two_one = pickle.loads(pickle.dumps(two))   # the same fitted model, served by ONE context
    two_one.devices = None
    Ey0, Vy0 = two_one.predict_moments(Xq)
    # rows are independent: sharding the query changes nothing, bit for bit
    assert np.array_equal(Ey1, Ey0) and np.array_equal(Vy1, Vy0)
    assert np.array_equal(two.predict(Xq), two_one.predict(Xq))
    # validation of the query reaches the caller's rows from every shard
    bad = Xq.copy()
    bad[-5, 1] = np.nan
    with pytest.raises(ValueError):
        two.predict_moments(bad)
    with pytest.raises(ValueError):
        two.predict(bad)
    # a concatenation takes the same route.  (Its L-BFGS-B path is not compared with the one-context fit's: from this start
    # the one-context run ends after a failed line search at the initial length scales while the sharded one -- whose `_elbo`
    # agrees with it to 1e-9 at any point, see test_sharded_elbo_equals_the_one_context_elbo -- walks on; what a fit must
    # deliver is an objective no worse than its start and a model that serves.)
    def cat():
        return bs.RandomMatern52(nbases=96, Xdim=d, random_state=2, lenscale=Parameter(np.ones(d), Positive())) + bs.LinearBasis(onescol=True)
    c2 = SLM(cat(), nstarts=0, maxiter=15, random_state=0, devices=[0, 0, 0, 0])
    c2.obj_ = -np.inf
    c2._state = c2._make_state(X.astype(np.float64), y.astype(np.float64))
    start = -c2._elbo(X, y, 1.0, [1.0, 1.0], np.ones(d))[0]
    c2._state.release()
    c2._state = None
    c2.fit(X, y)
    assert c2.obj_ >= start
    e2, v2 = c2.predict_moments(Xq[:30_001])
    c1 = pickle.loads(pickle.dumps(c2))
    c1.devices = None
    e1, v1 = c1.predict_moments(Xq[:30_001])
    assert normwise(e2, e1) < 1e-6 and normwise(v2, v1) < 1e-6 and np.all(v2 > 0)


def test_sklearn_protocol_with_devices():
    """clone / get_params / pickle keep ``devices``; a Pipeline + GridSearchCV (the reference's tests/test_models.py:39-80
    pattern) drives the multi-GPU fit without any launcher."""
    from sklearn.base import clone
    from sklearn.model_selection import GridSearchCV
    from sklearn.pipeline import make_pipeline
    from sklearn.preprocessing import StandardScaler
    bs, _hip, multigpu, Parameter, Positive, SLM = _setup()
    X, y = _data(3000, 4, seed=11)
    basis = bs.RandomRBF(nbases=32, Xdim=4, random_state=0)
    est = SLM(basis, nstarts=0, maxiter=10, devices=[0, 0])
    assert clone(est).get_params()["devices"] == [0, 0]
    fitted = pickle.loads(pickle.dumps(est.fit(X, y)))
    assert fitted.devices == [0, 0] and np.all(np.isfinite(fitted.predict(X[:100])))
    pipe = make_pipeline(StandardScaler(), SLM(basis, nstarts=0, maxiter=10, devices=[0, 0]))
    gs = GridSearchCV(pipe, {"standardlinearmodel__var": [Parameter(1.0, Positive()), Parameter(2.0, Positive())]}, cv=2, n_jobs=1)
    gs.fit(X, y)
    assert np.all(np.isfinite(gs.predict(X[:50])))
    # fewer rows than members can share: one GPU, quietly
    tiny = SLM(bs.RandomRBF(nbases=8, Xdim=4, random_state=0), nstarts=0, maxiter=3, devices=[0, 0, 0, 0]).fit(X[:6], y[:6])
    assert np.all(np.isfinite(tiny.weights_))


def test_bench_single_process_line():
    """`python bench.py --gpus 2 --single-process`: ONE JSON line of the contract's shape, the headline step on an in-process
    device group (members share this box's GPU: "oversubscribed", peer transport), the sharded `_elbo` with its oracle parity,
    the preflight of config 3's message -- and (forced here; on a node with a GPU per member it runs by itself next to RCCL)
    the same message through the library's own peer transport with its exact-sum check."""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    env = dict(os.environ, RR_BENCH_FORCE_PEER_PREFLIGHT="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--single-process", "--steps", "2",
                        "--warmup", "1", "--rows", "600000", "--dist-rows", "40000", "--full"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1 and len(lines[0]) < 8192, lines
    out = json.loads(lines[0])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data", "config", "roofline"):
        assert k in out, k
    assert out["n_gpus"] == 2 and out["config"]["single_process"] and out["config"]["members_bit_identical"]
    assert out["config"]["trace_rel_err"] < 1e-6 and out["value"] > 0
    ex = out["exchange"]
    assert ex["transport"] == "peer" and ex["oversubscribed"] and ex["distinct_gpus"] == 1 and ex["peer_access"]
    assert ex["message_bytes"] == 8 * (4096 * 4097 // 2 + 4096 + 2) and ex["preflight"]["busbw_GBps"] > 0
    pp = ex["preflight_peer_transport"]
    assert "error" not in pp and pp["sum_exact"] and pp["busbw_GBps"] > 0
    c = out["configs"]["elbo_rbf_f4096_single_process"]
    assert "error" not in c, c
    assert c["parity"]["members_bit_identical"] and c["parity"]["neg_elbo_256_rows"] < 1e-5 and c["parity"]["gradient_256_rows"] < 1e-3
    # config 5's SVI step with the loop resident on both members (rr_glm_sgd_group_step) next to the one-context fit
    g = out["configs"]["C5_glm_svi_step_single_process"]
    assert "error" not in g, g
    assert g["parity"]["params_after_8_steps_vs_one_context"] < 1e-4 and g["ms"] > 0 and g["one_context_ms"] > 0


def test_glm_with_devices_matches_the_one_context_run():
    """`GeneralizedLinearModel(devices=[...])`: the resident rows of X sharded over the members, every minibatch served by
    the members its row indices fall on, the step's sums added over them (glm.py:205-322).  Same seed -> the same minibatch
    stream and the same draws as the one-context run: ONE `_elbo` agrees to float32 rounding (the row sums regroup), and a
    short `fit` walks to the same parameters; latent-function samples of the fitted model shard over the query rows."""
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd.btypes import Parameter, Positive
    from revrand_amd.glm import GeneralizedLinearModel
    from revrand_amd.utils import flatten_values
    rs = np.random.RandomState(3)
    N, d, n, K, L, M = 40_000, 6, 64, 4, 20, 8192
    X = rs.randn(N, d).astype(np.float32)
    y = rs.poisson(np.exp(0.4 * X[:, 0] - 0.2 * X[:, 1])).astype(np.float64)
    F = 2 * n
    m, C = 0.1 * rs.randn(F, K), rs.gamma(2., 0.5, size=(F, K))
    ls = np.linspace(0.8, 1.5, d)

    def make(devices, maxiter=25):
        basis = bs.RandomRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
        return GeneralizedLinearModel(lk.Poisson(), basis, K=K, nsamples=L, batch_size=M, maxiter=maxiter, nstarts=0,
                                      random_state=2, devices=devices)
    evals = {}
    for devices in (None, [0, 0], [0, 0, 0, 0]):
        glm = make(devices)
        glm.B_, glm.D_ = N / M, F
        glm._GeneralizedLinearModel__it = 0   # (a logging iteration: the objective is evaluated, not only its gradient)
        feats = glm._features()
        assert type(feats).__name__ == ("MinibatchFeatures" if devices is None else "ShardedMinibatchFeatures")
        glm._resident_fit = feats.make_resident(X)
        assert glm._resident_fit
        idx = np.random.RandomState(5).permutation(N)[:M]
        f, g = glm._elbo(m, C, 1.3, [], ls, np.empty((M, 0)), y[idx], idx)
        evals[str(devices)] = np.concatenate(([f], flatten_values(g)))
        if devices is not None:
            assert feats.n_use == min(len(devices), M // feats.MIN_ROWS_PER_MEMBER) and len(feats._parts) == feats.n_use
        glm._resident_fit = False
        glm._release_features()
    ref = evals["None"]
    for k, v in evals.items():
        assert abs(v[0] - ref[0]) < 1e-5 * abs(ref[0]) and normwise(v[1:], ref[1:]) < 2e-4, k
    # (the start point of a fit is a draw from NumPy's GLOBAL stream, as in the reference: decorators.py:216-220)
    np.random.seed(77)
    one = make(None).fit(X, y)
    np.random.seed(77)
    two = make([0, 0]).fit(X, y)
    assert normwise(two.weights_, one.weights_) < 5e-3 and normwise(two.covariance_, one.covariance_) < 5e-3
    assert normwise(np.atleast_1d(two.basis_hypers_), np.atleast_1d(one.basis_hypers_)) < 5e-3
    Xq = rs.randn(9001, d).astype(np.float32)
    two.random_ = np.random.RandomState(9)
    one.random_ = np.random.RandomState(9)
    one.weights_, one.covariance_, one.basis_hypers_ = two.weights_, two.covariance_, two.basis_hypers_
    assert np.array_equal(two.predict(Xq, nsamples=20), one.predict(Xq, nsamples=20))   # rows are independent
