"""Spectral-mixture components (FastFoodGM, basis_functions.py:1386-1562) in the wide small-minibatch loop
(rr_glm_sviwgm_create, rr_svi_wide.hip; ``GeneralizedLinearModel(resident_bases="all", fused_bases="all+gm", wide_fused=True)``).

* T1 - T3: the mixed case of tests/gm_cases.py -- linear | GM (d = 3, a zero and a negative mean) | random Fourier ARD | GM (d = 1),
  Gaussian, F = 70 -- through _hip.WideSvi(..., gm_children=True) against the float64 oracle (oracle.glm_elbo on the dense
  restatement of the component): one plain SGD step at two cuts into items, four Adam steps with the log trick, five random starts;
* T4: the widest slots: one component on 128 columns (256 slots = the most a child can own) next to a linear child, K = 2 and K = 1;
* T5: bits: reruns, run(4) against four run(1), blocks of steps and chunks of random starts through GeneralizedLinearModel;
* T6: whole fits: wide == the step-per-call loop == the host loop around `_elbo`; T7: the device sampler;
* T8: routing without the tests' switch; T9: the launches of a step.

Bounds (the project's for the same comparisons in tests/test_gpu_fused_svi_gm.py): 1e-6 normwise per block against the float64
oracle -- both sides float64 on identical inputs, the draws rounded to float32 once; 1e-4 between loops -- the other loops form
float32 features.

Measured on an MI355X (docs/KERNELS.md 3.50): see the table there."""
import numpy as np
import pytest

import gm_cases as gc
from conftest import normwise
from test_gpu_fused_wide import KERNELS, UPDATERS, _Spies

pytestmark = pytest.mark.gpu

TOL = 1e-6
FIT_TOL = 1e-4


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd import optimize as opt
    from revrand_amd.btypes import Bound, Parameter, Positive
    from revrand_amd.glm import GeneralizedLinearModel
    return bs, lk, opt, Bound, Parameter, Positive, GeneralizedLinearModel


class _Wide(object):
    """_hip.WideSvi(..., gm_children=True) on host arrays: uploads, runs, frees."""

    def __init__(self, children, y, K, L, M, lik, n_lik, z0, updater, par, maxiter, bmag, lower=None, upper=None, is_log=None):
        from revrand_amd import _hip
        self.dev = _hip.get_device()
        self.bufs = []
        kids = []
        for ch in children:   # (kind, ..., X columns as a float64 host matrix)
            dX = self.dev.upload_matrix(np.ascontiguousarray(ch[-1], dtype=np.float64))
            self.bufs.append(dX)
            kids.append(tuple(ch[:-1]) + (dX,))
        dy = self.dev.upload_vector(y, np.float64)
        self.bufs.append(dy)
        n = z0.size
        try:
            self.svi = _hip.WideSvi(self.dev, kids, len(y), dy, None, None, K, L, M, lik, n_lik, z0,
                                    np.full(n, -np.inf) if lower is None else lower, np.full(n, np.inf) if upper is None else upper,
                                    np.zeros(n, dtype=bool) if is_log is None else is_log, _hip.UPDATER_IDS[updater], par, maxiter,
                                    bmag, gm_children=True)
        except Exception:
            self.free()
            raise

    def up(self, arr, dtype):
        b = self.dev.upload_vector(np.ascontiguousarray(arr, dtype=dtype))
        self.bufs.append(b)
        return b

    def free(self):
        for b in self.bufs:
            b.free()
        self.bufs = []

    def close(self):
        self.svi.close()
        self.free()


@pytest.fixture(scope="module")
def mixed():
    return gc.Mixed()


@pytest.fixture(scope="module")
def mixed_step(mixed):
    """oracle.glm_elbo of the mixed case's first minibatch at x0: made once, shared, never changed"""
    obj, ref = mixed.elbo(mixed.x0, mixed.idx[0], mixed.e[0])
    ref.setflags(write=False)
    return obj, ref


def _handles(c):
    from revrand_amd import _hip
    return tuple(_hip.RffHandle(np.ascontiguousarray(W)) for W in (c.V1, c.W, c.V2))


def _item(monkeypatch, item):
    if item is None:
        monkeypatch.delenv("RR_SVIW_ITEM", raising=False)
    else:
        monkeypatch.setenv("RR_SVIW_ITEM", item)


# ---- T1 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("item", ["3", None])
def test_mixed_children_one_step_against_the_oracle(mixed, mixed_step, monkeypatch, item):
    """one plain SGD step without the log trick: (z0 - z1) / eta IS the gradient the chain formed, objs[0] the step's -ELBO.
    RR_SVIW_ITEM=3: the components are cut 3,3,2 and 3,2, the Fourier child 3,3; unset: one item per child.  Each cut is held to
    the oracle on its own; the four mean gradients asserted apart from the nine length-scale gradients."""
    from revrand_amd import likelihoods as lk
    c = mixed
    _item(monkeypatch, item)
    eta = 1e-4
    run = _Wide(c.children(*_handles(c)), c.y, c.K, c.L, c.M, lk.RR_LIK_GAUSSIAN, 1, c.x0, "SGDUpdater", [eta], 1, c.B)
    try:
        run.svi.run(1, run.up(c.idx[0], np.int32), run.up(c.e[0].reshape(c.K * c.L, c.F), np.float32))
        z1, objs, norms = run.svi.read()
    finally:
        run.close()
    obj, ref = mixed_step
    got = (c.x0 - z1) / eta
    # ((z0 - z1) / eta cancels: |z| ~ 1 leaves 2e-16 / eta = 2e-12 absolute on gradients of magnitude >= 1e-2 -- far below 1e-6)
    e = (abs(objs[0] - obj) / abs(obj),) + tuple(normwise(u, v) for u, v in zip(c.blocks(got), c.blocks(ref)))
    print("wide GM, item %s, one step vs oracle: obj %.2e dm %.2e dC %.2e dL %.2e dvar %.2e dmean %.2e dls %.2e" % ((item,) + e))
    assert abs(norms[0] - np.linalg.norm(ref)) < TOL * np.linalg.norm(ref)
    assert e[5] < TOL, ("mean gradients", e[5], c.blocks(got)[4], c.blocks(ref)[4])
    assert e[6] < TOL, ("length-scale gradients", e[6], c.blocks(got)[5], c.blocks(ref)[5])
    assert all(v < TOL for v in e), e


# ---- T2 ------------------------------------------------------------------------------------------------------------------
def _adam_setup(c):
    pos = c.positive
    z0 = np.where(pos, np.log(np.where(pos, c.x0, 1.0)), c.x0)
    lower = np.where(pos, np.log(1e-14), -np.inf)
    upper = np.full(z0.size, np.inf)
    lower[c.mean_slots[3]], upper[c.mean_slots[3]] = -2.0, 2.0
    return pos, z0, lower, upper


def _adam_run(c, cuts):
    """four Adam steps over the four minibatches, queued as `cuts` calls of run: (z, objs, norms)"""
    from revrand_amd import likelihoods as lk
    pos, z0, lower, upper = _adam_setup(c)
    run = _Wide(c.children(*_handles(c)), c.y, c.K, c.L, c.M, lk.RR_LIK_GAUSSIAN, 1, z0, "Adam", [0.01, 0.9, 0.99, 1e-8], 4, c.B,
                lower=lower, upper=upper, is_log=pos)
    try:
        t = 0
        for n in cuts:
            run.svi.run(n, run.up(c.idx[t:t + n], np.int32), run.up(c.e[t:t + n].reshape(n, c.K * c.L, c.F), np.float32))
            t += n
        return run.svi.read()
    finally:
        run.close()


def test_mixed_children_four_adam_steps_with_the_log_trick(mixed, monkeypatch):
    """every positive coordinate in log space, the means in plain space with Bound(-2, 2) on the second component's; replayed with
    oracle.glm_elbo, the chain rule of the log trick (decorators.py:329-408), oracle.sgd_update and the clip (sgd.py:404-420)"""
    import revrand_oracle as orc
    c = mixed
    _item(monkeypatch, "3")
    pos, z0, lower, upper = _adam_setup(c)
    z4, objs, _ = _adam_run(c, (4,))
    z, state, ref_objs = z0.copy(), {}, []
    for t in range(4):
        x = np.where(pos, np.exp(np.where(pos, z, 0.0)), z)
        obj, gx = c.elbo(x, c.idx[t], c.e[t])
        gz = np.where(pos, gx * x, gx)
        gz = np.where((z <= lower) & (gz > 0), 0.0, gz)
        gz = np.where((z >= upper) & (gz < 0), 0.0, gz)
        z = np.clip(orc.sgd_update("adam", state, z, gz), lower, upper)
        ref_objs.append(obj)
    e = tuple(normwise(u, v) for u, v in zip(c.blocks(z4), c.blocks(z))) + (normwise(objs, np.array(ref_objs)),)
    print("wide GM, four Adam steps vs oracle: m %.2e logC %.2e log reg %.2e log var %.2e mean %.2e log ls %.2e objs %.2e" % e)
    assert np.abs(z4 - z0).max() > 0.02   # (the steps moved the parameters)
    assert np.all(np.abs((z4 - z0)[c.mean_slots]) > 1e-3)   # ... the means among them, the one that started at zero too
    assert all(v < TOL for v in e), e


# ---- T3 ------------------------------------------------------------------------------------------------------------------
def test_mixed_children_random_starts_against_the_oracle(mixed, monkeypatch):
    """WideSvi.starts on five candidates, each on a minibatch and draws of its own (the fifth takes the first's again)"""
    from revrand_amd import likelihoods as lk
    c = mixed
    _item(monkeypatch, "3")
    rs = np.random.RandomState(3)
    cands = np.stack([np.where(c.positive, c.x0 * np.exp(0.2 * rs.randn(c.x0.size)), c.x0 + 0.1 * rs.randn(c.x0.size)) for _ in range(5)])
    pick = [0, 1, 2, 3, 0]
    run = _Wide(c.children(*_handles(c)), c.y, c.K, c.L, c.M, lk.RR_LIK_GAUSSIAN, 1, c.x0, "Adam", [0.01, 0.9, 0.99, 1e-8], 1, c.B)
    try:
        got = run.svi.starts(run.up(c.idx[pick], np.int32), cands, run.up(c.e[pick].reshape(5, c.K * c.L, c.F), np.float32))
    finally:
        run.close()
    ref = np.array([c.elbo(cands[i], c.idx[pick[i]], c.e[pick[i]])[0] for i in range(5)])
    e = np.abs(got - ref) / np.abs(ref)
    print("wide GM, random starts vs oracle:", e)
    assert len(set(np.round(ref, 6))) == 5 and np.all(e < TOL), (got, ref)
    assert int(np.argmin(got)) == int(np.argmin(ref))


# ---- T4 ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 1])
def test_one_component_on_128_columns_fills_every_slot(K):
    """linear (3 columns + ones) | GM on 128 columns, V = randn(128, 6): n_ls = 256 = the most slots a child can own; L = 5,
    M = 7, Gaussian; one plain SGD step against oracle.glm_elbo on gm_transform / gm_grad"""
    import revrand_oracle as orc
    from revrand_amd import _hip
    from revrand_amd import likelihoods as lk
    rs = np.random.RandomState(41)
    N, d, n, L, M = 35, 128, 6, 5, 7
    Xg, Xl = 0.3 * rs.randn(N, d), rs.randn(N, 3)
    y = np.sin(Xl[:, 0]) + 0.1 * rs.randn(N)
    V = rs.randn(d, n)
    F = 4 + 4 * n
    m, C = 0.3 * rs.randn(F, K), rs.gamma(2., 0.5, size=(F, K))
    regs, var = np.array([1.3, 0.8]), 0.45
    mean, ls = 0.2 * rs.randn(d), rs.uniform(0.8, 1.5, size=d)
    mean[5] = 0.0
    x0 = np.concatenate([m.ravel(), C.ravel(), regs, [var], mean, ls])
    idx = rs.permutation(N)[:M].astype(np.int32)
    e = rs.randn(K, L, F).astype(np.float32)
    B = N / float(M)
    eta = 1e-4
    run = _Wide([("linear", 3, True, Xl), ("gm", _hip.RffHandle(np.ascontiguousarray(V)), 2 * d, Xg)], y, K, L, M, lk.RR_LIK_GAUSSIAN, 1,
                x0, "SGDUpdater", [eta], 1, B)
    try:
        run.svi.run(1, run.up(idx, np.int32), run.up(e.reshape(K * L, F), np.float32))
        z1, objs, norms = run.svi.read()
    finally:
        run.close()
    slices = [slice(0, 4), slice(4, F)]
    Phi = np.hstack([orc.linear_transform(Xl[idx], True), gc.gm_transform(Xg[idx], V, mean, ls)])
    dm, dl = gc.gm_grad(Xg[idx], V, mean, ls)

    def slab(block):
        out = np.zeros_like(Phi)
        out[:, slices[1]] = block
        return out
    dPhis = [slab(dm[:, :, i]) for i in range(d)] + [slab(dl[:, :, i]) for i in range(d)]
    rd = np.concatenate([np.full(4, regs[0]), np.full(4 * n, regs[1])])
    obj, (ndm, ndC, dL, dlp, dbp) = orc.glm_elbo(m, C, rd, slices, "gaussian", [var], (), Phi, dPhis, y[idx], np.asarray(e, dtype=np.float64), B)
    ref = np.concatenate([ndm.ravel(), ndC.ravel(), np.ravel(dL), np.ravel(dlp), np.ravel(dbp)])
    got = (x0 - z1) / eta
    fk = F * K
    cut = [0, fk, 2 * fk, 2 * fk + 2, 2 * fk + 3, 2 * fk + 3 + d, 2 * fk + 3 + 2 * d]
    errs = (abs(objs[0] - obj) / abs(obj),) + tuple(normwise(got[a:b], ref[a:b]) for a, b in zip(cut[:-1], cut[1:]))
    print("wide GM, 128 columns, K = %d: obj %.2e dm %.2e dC %.2e dL %.2e dvar %.2e dmean %.2e dls %.2e" % ((K,) + errs))
    assert got.size == cut[-1] and np.all(np.abs(ref[cut[4]:]) > 0)
    assert all(v < TOL for v in errs), errs


# ---- fits ----------------------------------------------------------------------------------------------------------------
def _data(lik, d, N=300, seed=4):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, d)
    f = 0.5 * np.sin(X[:, 0]) + 0.2 * X[:, 2]
    if lik == "poisson":
        return X, rs.poisson(np.exp(f)).astype(float)
    return X, f + 0.1 * rs.randn(N)


def _basis(name):
    """(basis, Xdim)"""
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()

    def gm(nbases, d, seed, mean, ls):
        return bs.FastFoodGM(nbases=nbases, Xdim=d, random_state=seed, mean=Parameter(mean * np.ones(d), Bound()),
                             lenscale=Parameter(ls * np.ones(d), Positive()))
    if name == "gm12":     # the chain's mixture mode serves the other loops
        return gm(16, 12, 2, np.linspace(-0.3, 0.4, 12), 1.2), 12
    if name == "gm3":      # the dense equivalent serves them (rr_featmat_put_gm)
        return gm(8, 3, 2, np.linspace(-0.3, 0.4, 3), 1.2), 3
    if name == "cat3":
        return bs.LinearBasis(onescol=True) + gm(8, 3, 5, np.array([0.5, 0.0, -0.2]), 0.9) \
            + bs.RandomRBF(nbases=6, Xdim=3, random_state=3, lenscale=Parameter(np.ones(3), Positive())), 3
    if name == "four32":   # four nbases=32 components on Xdim = 4: F = 512
        b = gm(32, 4, 1, np.linspace(-0.3, 0.4, 4), 1.2)
        for s in (2, 3, 4):
            b = b + gm(32, 4, s, np.linspace(-0.2, 0.3, 4) * s, 0.8 + 0.1 * s)
        return b, 4
    if name == "one32":
        return gm(32, 4, 1, np.linspace(-0.3, 0.4, 4), 1.2), 4
    raise KeyError(name)


def _flat(v):
    if isinstance(v, (list, tuple)):
        return np.concatenate([_flat(u) for u in v]) if len(v) else np.empty(0)
    return np.atleast_1d(np.asarray(v, dtype=float)).ravel()


def _fit(loop, basis, lik="poisson", updater=None, sampler="host", maxiter=12, K=4, L=10, batch=10, nstarts=3, block=None,
         block_bytes=None, record=None, force=True, fused_bases="all+gm", wide_fused=None, devices=None):
    """loop: "wide" (fused_bases="all+gm", wide_fused=True and the tests' switch), "resident" (the step-per-call loop), "host"
    (optimize.sgd around `_elbo`)"""
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    from revrand_amd import glm as glm_mod
    b, d = _basis(basis)
    X, y = _data(lik, d)
    like = {"poisson": lk.Poisson, "gaussian": lk.Gaussian}[lik]()
    glm = GLM(like, b, K=K, nsamples=L, batch_size=batch, maxiter=maxiter, nstarts=nstarts, random_state=11,
              updater=UPDATERS[updater](opt) if updater is not None else None, sampler=sampler, resident_bases="all",
              fused_bases=fused_bases, wide_fused=(loop == "wide") if wide_fused is None else wide_fused, devices=devices)
    glm._resident_sgd = loop != "host"
    glm._fused_sgd = loop == "wide"
    glm._wide_fused_force = force and loop == "wide"
    saved = (glm_mod._FusedLoop.BLOCK_STEPS, glm_mod._FusedLoop.BLOCK_BYTES)
    if block is not None:
        glm_mod._FusedLoop.BLOCK_STEPS = block
    if block_bytes is not None:
        glm_mod._FusedLoop.BLOCK_BYTES = block_bytes
    try:
        with _Spies(record) as calls:
            np.random.seed(3)
            glm.fit(X, y)
    finally:
        glm_mod._FusedLoop.BLOCK_STEPS, glm_mod._FusedLoop.BLOCK_BYTES = saved
    out = (glm.weights_.copy(), glm.covariance_.copy(), _flat(glm.regularizer_), _flat(glm.like_hypers_), _flat(glm.basis_hypers_),
           glm.random_.randn())
    return out, dict(calls)


def _ran_wide(calls, steps, starts):
    assert calls["wide"] == steps and calls["wide_starts"] == starts and calls["fused"] == 0 and calls["resident"] == 0, calls


def _same(a, b, tol, what):
    errs = [normwise(u, v) for u, v in zip(a[:5], b[:5]) if u.size]
    print("%s: worst block %.3e (bound %.0e)" % (what, max(errs), tol))
    for u, v in zip(a[:5], b[:5]):
        assert u.shape == v.shape and np.all(np.isfinite(u))
    assert max(errs) < tol, (errs, tol)
    assert a[5] == b[5]   # the RandomState ends in the same state: same minibatches, same draws consumed


def _bits(a, b):
    for u, v in zip(a[:5], b[:5]):
        assert np.array_equal(u, v)
    assert a[5] == b[5]


# ---- T5: bits ------------------------------------------------------------------------------------------------------------
def test_reruns_and_cuts_into_calls_are_bit_identical(mixed, monkeypatch):
    _item(monkeypatch, "3")
    whole = _adam_run(mixed, (4,))
    again = _adam_run(mixed, (4,))
    single = _adam_run(mixed, (1, 1, 1, 1))
    for u, v, w in zip(whole, again, single):
        assert np.array_equal(u, v) and np.array_equal(u, w)
    assert whole[1].shape == (4,) and np.all(np.isfinite(whole[1])) and np.all(whole[2] > 0)


def test_blocks_of_steps_and_chunks_of_starts_are_bit_identical_through_the_model():
    first, c = _fit("wide", "cat3", "gaussian")
    _ran_wide(c, 12, 3)
    for block, runs in ((1, 12), (7, 2), (256, 1)):
        cut, cc = _fit("wide", "cat3", "gaussian", block=block)
        assert cc["wide_runs"] == runs and cc["wide"] == 12
        _bits(first, cut)
        for u, v in zip(c["read"], cc["read"]):
            assert np.array_equal(u, v)
    # BLOCK_BYTES lowered so that 5 candidates take 3 chunks
    K, L, F = 4, 10, first[0].shape[0]
    per = (2 * F * K + first[2].size + first[3].size + first[4].size) * 8 + K * L * F * 4
    rec1, rec2 = [], []
    whole, c1 = _fit("wide", "cat3", "gaussian", nstarts=5, maxiter=5, record=rec1)
    cut, c2 = _fit("wide", "cat3", "gaussian", nstarts=5, maxiter=5, record=rec2, block_bytes=2 * per + 16)
    assert c1["start_calls"] == 1 and c2["start_calls"] == 3 and c1["wide_starts"] == c2["wide_starts"] == 5
    a, b = np.concatenate(rec1), np.concatenate(rec2)
    assert np.array_equal(a, b) and int(np.argmin(a)) == int(np.argmin(b))
    _bits(whole, cut)


# ---- T6: whole fits ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("basis, lik, updater", [("gm12", "poisson", None), ("gm3", "gaussian", "AdaDelta"),
                                                 ("cat3", "gaussian", None), ("cat3", "poisson", "AdaGrad")])
def test_wide_loop_equals_the_other_two(basis, lik, updater):
    """12 steps, K = 4, L = 10, batch 10, N = 300, three starts; updater None: the model's default, Adam"""
    wide, calls = _fit("wide", basis, lik, updater=updater)
    _ran_wide(calls, 12, 3)
    res, c = _fit("resident", basis, lik, updater=updater)
    assert c["resident"] == 12 and c["wide"] == 0 and c["fused"] == 0 and c["wide_starts"] == 0, c
    host, c = _fit("host", basis, lik, updater=updater)
    assert c["resident"] == 0 and c["wide"] == 0 and c["fused"] == 0 and c["wide_starts"] == 0, c
    _same(wide, res, FIT_TOL, "%s %s %s wide vs step-per-call" % (basis, lik, updater))
    _same(wide, host, FIT_TOL, "%s %s %s wide vs host" % (basis, lik, updater))


# ---- T7: the device sampler ------------------------------------------------------------------------------------------------
def test_device_sampler_equals_the_step_per_call_loop():
    """sampler="device": both device loops see the kernel generator's draws, the same function of (seed, step, sample, feature)"""
    for basis, lik in (("gm12", "poisson"), ("cat3", "gaussian")):
        wide, calls = _fit("wide", basis, lik, sampler="device")
        _ran_wide(calls, 12, 3)
        res, c = _fit("resident", basis, lik, sampler="device")
        assert c["resident"] == 12 and c["wide"] == 0 and c["fused"] == 0, c
        _same(wide, res, FIT_TOL, "%s %s device sampler" % (basis, lik))


# ---- T8: routing, unforced --------------------------------------------------------------------------------------------------
REPORT = dict(K=10, L=50, batch=10, maxiter=6, nstarts=2, force=False)


def test_four_components_take_the_wide_loop():
    """four FastFoodGM(nbases=32) components on Xdim = 4 (F = 512) at the reference's K = 10, 50 samples, 10 rows: outside the
    LDS kernel's range for spectral-mixture children -- the shape that kept the step-per-call loop before"""
    out, calls = _fit("wide", "four32", "gaussian", **REPORT)
    assert out[0].shape == (512, 10)
    _ran_wide(calls, 6, 2)
    many, c2 = _fit("wide", "four32", "gaussian", devices=[0, 0], **REPORT)     # a device group: the wide loop on member 0
    _ran_wide(c2, 6, 2)
    _bits(out, many)


def test_other_keyword_pairs_route_as_before():
    """wide_fused=False: the step-per-call loop.  fused_bases="all": no spectral-mixture child in any fused loop -- and on
    Xdim = 4 <= 8 the chain's mixture mode does not serve the component, so there are no resident rows either: the host loop, as
    before (tests/test_gpu_fused_svi_gm.py::test_without_the_opt_in_three_columns_run_no_device_loop).  A lone component at
    K = 3, L = 10 still takes the LDS kernel."""
    out, calls = _fit("wide", "four32", "gaussian", wide_fused=False, **REPORT)
    assert calls["resident"] == 6 and calls["wide"] == 0 and calls["fused"] == 0 and calls["wide_starts"] == 0, calls
    out, calls = _fit("wide", "four32", "gaussian", fused_bases="all", **REPORT)
    assert calls["wide"] == 0 and calls["fused"] == 0 and calls["wide_starts"] == 0, calls
    out, calls = _fit("wide", "one32", "gaussian", K=3, L=10, maxiter=6, nstarts=2, force=False)
    assert calls["fused"] == 6 and calls["wide"] == 0 and calls["resident"] == 0 and calls["wide_starts"] == 0, calls


# ---- T9: the launches of a step (the bounds-checking build counts them: tests/test_gpu_fused_wide_gm_debug.py) ----------------
def test_launches_per_step_and_per_candidate():
    """n steps are n x (A, B, C, D), n candidates n x (A, B, D), spectral-mixture items or not: the four kernels keep their names"""
    from revrand_amd import _hip
    lib = _hip.load_library()
    debug = bool(lib.rr_build_flags() & 1)
    lib.rr_debug_kernel_launches(None)
    out, calls = _fit("wide", "cat3", "poisson", maxiter=9, nstarts=4, block=4)
    _ran_wide(calls, 9, 4)
    counts = [lib.rr_debug_kernel_launches(k.encode()) for k in KERNELS]
    if debug:
        assert counts == [9 + 4, 9 + 4, 9, 9 + 4], counts
        assert lib.rr_debug_kernel_launches(b"rr_glm_svi_steps_kernel") == 0
    else:
        assert counts == [-1] * 4
