"""Spectral-mixture components (FastFoodGM, basis_functions.py:1386-1562) in the many-steps-per-launch kernel of small
minibatches (rr_glm_svi_create_gm, rr_svi.hip; ``GeneralizedLinearModel(resident_bases="all", fused_bases="all+gm")``).

* T2: the mixed case of tests/gm_cases.py -- linear | GM (d = 3, a zero and a negative mean) | random Fourier ARD | GM (d = 1),
  Gaussian -- against the float64 oracle (oracle.glm_elbo on the dense restatement of the component, which
  tests/test_fused_gm_host.py holds to the reference's recorded values): one step, four Adam steps with the log trick on the
  positive coordinates and the means in plain space, the batched random starts;
* T3: whole fits: fused == the step-per-call resident loop == the host loop around `_elbo`, for Xdim = 12 (the chain's mixture
  mode serves the other two loops), Xdim = 3 and Xdim = 1 (the dense equivalent serves them: rr_featmat_put_gm);
* T4: launches of 7 steps and reruns give the same bits, the device sampler, the device-group path, what stays on the
  step-per-call loop, refusals.

T2's bound is 1e-6: both sides evaluate the same function in float64 on identical inputs (the draws rounded to float32 once) --
the project's bound for this kernel's other children against the float64 oracle (tests/test_gpu_fused_svi_centres.py).  T3's is
1e-4: the other two loops form float32 features with the mean shift; the project's bound for GM children between those loops
at 12 steps (tests/test_gpu_resident_sgd.py::test_spectral_mixture_children_run_resident).

Measured on an MI355X (docs/KERNELS.md 3.40): T2 one step <= 9.9e-14 in every block (means 6.0e-14, length scales 9.9e-14), four
Adam steps <= 2.1e-16, random starts <= 3.5e-16; T3 fits <= 9.1e-8, device sampler <= 6.0e-8."""
import numpy as np
import pytest

import gm_cases as gc
from conftest import normwise

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


def _oracle():
    import revrand_oracle as orc
    return orc


class _Svi(object):
    """_hip.FusedSvi(..., gm_children=True) on host arrays: uploads, runs, frees."""

    def __init__(self, children, y, K, L, M, lik, n_lik, z0, updater, par, maxiter, bmag, lower=None, upper=None, is_log=None,
                 **how):
        from revrand_amd import _hip
        self.hip, self.dev = _hip, _hip.get_device()
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
            self.svi = _hip.FusedSvi(self.dev, kids, len(y), dy, None, None, K, L, M, lik, n_lik, z0,
                                     np.full(n, -np.inf) if lower is None else lower, np.full(n, np.inf) if upper is None else upper,
                                     np.zeros(n, dtype=bool) if is_log is None else is_log, _hip.UPDATER_IDS[updater], par, maxiter,
                                     bmag, **(how or dict(gm_children=True)))
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


def _handles(c):
    from revrand_amd import _hip
    return tuple(_hip.RffHandle(np.ascontiguousarray(W)) for W in (c.V1, c.W, c.V2))


# ---- T2 ------------------------------------------------------------------------------------------------------------------

def test_mixed_children_one_step_against_the_oracle(mixed):
    """(1) one plain SGD step without the log trick: (z0 - z1) / eta IS the gradient the kernel formed, objs[0] the step's -ELBO;
    the four mean gradients asserted apart from the nine length-scale gradients"""
    from revrand_amd import likelihoods as lk
    c = mixed
    eta = 1e-4
    run = _Svi(c.children(*_handles(c)), c.y, c.K, c.L, c.M, lk.RR_LIK_GAUSSIAN, 1, c.x0, "SGDUpdater", [eta], 1, c.B)
    try:
        run.svi.run(1, run.up(c.idx[0], np.int32), run.up(c.e[0].reshape(c.K * c.L, c.F), np.float32))
        z1, objs, norms = run.svi.read()
    finally:
        run.close()
    obj, ref = c.elbo(c.x0, c.idx[0], c.e[0])
    got = (c.x0 - z1) / eta
    # ((z0 - z1) / eta cancels: |z| ~ 1 leaves 2e-16 / eta = 2e-12 absolute on gradients of magnitude >= 1e-2 -- far below 1e-6)
    e = (abs(objs[0] - obj) / abs(obj),) + tuple(normwise(u, v) for u, v in zip(c.blocks(got), c.blocks(ref)))
    print("GM mixed children, one step vs oracle: obj %.2e dm %.2e dC %.2e dL %.2e dvar %.2e dmean %.2e dls %.2e" % e)
    print("   mean gradients (oracle):", np.array2string(c.blocks(ref)[4], precision=3))
    print("   length-scale gradients (oracle):", np.array2string(c.blocks(ref)[5], precision=3))
    assert abs(norms[0] - np.linalg.norm(ref)) < TOL * np.linalg.norm(ref)
    assert e[5] < TOL, ("mean gradients", e[5], c.blocks(got)[4], c.blocks(ref)[4])
    assert e[6] < TOL, ("length-scale gradients", e[6], c.blocks(got)[5], c.blocks(ref)[5])
    assert all(v < TOL for v in e), e


def test_mixed_children_four_adam_steps_with_the_log_trick(mixed):
    """(2) four Adam steps over four minibatches, every positive coordinate in log space, the means in plain space with
    Bound(-2, 2) on the second component's; replayed with oracle.glm_elbo, the chain rule of the log trick
    (decorators.py:329-408), oracle.sgd_update and the clip (sgd.py:404-420)"""
    from revrand_amd import likelihoods as lk
    orc = _oracle()
    c = mixed
    pos = c.positive
    z0 = np.where(pos, np.log(np.where(pos, c.x0, 1.0)), c.x0)
    lower = np.where(pos, np.log(1e-14), -np.inf)
    upper = np.full(z0.size, np.inf)
    lower[c.mean_slots[3]], upper[c.mean_slots[3]] = -2.0, 2.0
    run = _Svi(c.children(*_handles(c)), c.y, c.K, c.L, c.M, lk.RR_LIK_GAUSSIAN, 1, z0, "Adam", [0.01, 0.9, 0.99, 1e-8], 4, c.B,
               lower=lower, upper=upper, is_log=pos)
    try:
        run.svi.run(4, run.up(c.idx, np.int32), run.up(c.e.reshape(4, c.K * c.L, c.F), np.float32))
        z4, objs, _ = run.svi.read()
    finally:
        run.close()
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
    print("GM mixed children, four Adam steps vs oracle: m %.2e logC %.2e log reg %.2e log var %.2e mean %.2e log ls %.2e objs %.2e" % e)
    assert np.abs(z4 - z0).max() > 0.02   # (the steps moved the parameters)
    assert np.all(np.abs((z4 - z0)[c.mean_slots]) > 1e-3)   # ... the means among them, the one that started at zero too
    assert all(v < TOL for v in e), e


def test_mixed_children_random_starts_against_the_oracle(mixed):
    """(3) FusedSvi.starts on three candidates, each on its own minibatch with its own draws: oracle.glm_elbo's objective"""
    from revrand_amd import likelihoods as lk
    c = mixed
    rs = np.random.RandomState(3)
    cands = np.stack([np.where(c.positive, c.x0 * np.exp(0.2 * rs.randn(c.x0.size)), c.x0 + 0.1 * rs.randn(c.x0.size)) for _ in range(3)])
    run = _Svi(c.children(*_handles(c)), c.y, c.K, c.L, c.M, lk.RR_LIK_GAUSSIAN, 1, c.x0, "Adam", [0.01, 0.9, 0.99, 1e-8], 1, c.B)
    try:
        got = run.svi.starts(run.up(c.idx[1:4], np.int32), cands, run.up(c.e[1:4].reshape(3, c.K * c.L, c.F), np.float32))
    finally:
        run.close()
    ref = np.array([c.elbo(cands[i], c.idx[1 + i], c.e[1 + i])[0] for i in range(3)])
    e = np.abs(got - ref) / np.abs(ref)
    print("GM mixed children, random starts vs oracle:", e)
    assert len(set(np.round(ref, 6))) == 3 and np.all(e < TOL), (got, ref)


# ---- T3: fits ------------------------------------------------------------------------------------------------------------

def _data(lik, N=500, d=4, seed=4):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, d)
    f = 0.5 * np.sin(X[:, 0]) + (0.2 * X[:, 2] if d > 2 else 0.0)
    if lik == "poisson":
        return X, rs.poisson(np.exp(f)).astype(float), ()
    return X, f + 0.1 * rs.randn(N), ()


def _basis(name, X):
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    d = X.shape[1]

    def gm(nbases, seed, mean, ls):
        return bs.FastFoodGM(nbases=nbases, Xdim=d, random_state=seed, mean=Parameter(mean * np.ones(d), Bound()),
                             lenscale=Parameter(ls * np.ones(d), Positive()))
    if name == "gm":       # one component alone
        return gm(16 if d > 8 else 8, 2, np.linspace(-0.3, 0.4, d) if d > 1 else 0.3, 1.2)
    if name == "cat":      # linear | two components | RandomRBF
        return bs.LinearBasis(onescol=True) + gm(8, 2, np.linspace(-0.3, 0.4, d), 1.2) + gm(8, 5, np.array([0.5, 0.0, -0.2]), 0.9) \
            + bs.RandomRBF(nbases=6, Xdim=d, random_state=3)
    raise KeyError(name)


def _fit(loop, basis, lik="poisson", sampler="host", maxiter=12, K=4, L=10, batch=10, nstarts=3, block=None, devices=None,
         fused_bases="all+gm", d=12):
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    from revrand_amd import _hip
    from revrand_amd import glm as glm_mod
    X, y, largs = _data(lik, d=d)
    like = {"poisson": lk.Poisson, "gaussian": lk.Gaussian}[lik]()
    glm = GLM(like, _basis(basis, X), K=K, nsamples=L, batch_size=batch, maxiter=maxiter, nstarts=nstarts, random_state=11,
              sampler=sampler, resident_bases="all", fused_bases=fused_bases, devices=devices)
    glm._resident_sgd = loop != "host"
    glm._fused_sgd = loop == "fused"
    if block is not None:
        old = glm_mod._FusedLoop.BLOCK_STEPS
        glm_mod._FusedLoop.BLOCK_STEPS = block
    calls = {"run": 0, "steps": 0, "starts": 0, "resident": 0}
    real_run, real_starts, real_step = _hip.FusedSvi.run, _hip.FusedSvi.starts, _hip.ResidentSgd.step

    def run(self, n, *a, **k):
        calls["run"] += 1
        calls["steps"] += n
        return real_run(self, n, *a, **k)

    def starts(self, didx, cand, *a, **k):
        calls["starts"] += len(cand)
        return real_starts(self, didx, cand, *a, **k)

    def step(self, *a, **k):
        calls["resident"] += 1
        return real_step(self, *a, **k)
    _hip.FusedSvi.run, _hip.FusedSvi.starts, _hip.ResidentSgd.step = run, starts, step
    try:
        np.random.seed(3)
        glm.fit(X, y, likelihood_args=largs)
    finally:
        _hip.FusedSvi.run, _hip.FusedSvi.starts, _hip.ResidentSgd.step = real_run, real_starts, real_step
        if block is not None:
            glm_mod._FusedLoop.BLOCK_STEPS = old

    def flat(v):
        if isinstance(v, (list, tuple)):
            return np.concatenate([flat(u) for u in v]) if len(v) else np.empty(0)
        return np.atleast_1d(np.asarray(v, dtype=float)).ravel()

    def shape(v):
        return [shape(u) for u in v] if isinstance(v, (list, tuple)) else (type(v).__name__, np.shape(v))
    return (glm.weights_.copy(), glm.covariance_.copy(), flat(glm.regularizer_), flat(glm.like_hypers_), flat(glm.basis_hypers_),
            glm.random_.randn(), shape(glm.basis_hypers_)), calls


def _same(a, b, tol, what=""):
    worst = max([normwise(u, v) for u, v in zip(a[:5], b[:5]) if u.size])
    print("%s: worst block %.3e (bound %.0e)" % (what, worst, tol))
    for u, v in zip(a[:5], b[:5]):
        assert u.shape == v.shape
        if u.size:
            assert np.all(np.isfinite(u)) and normwise(u, v) < tol, (normwise(u, v), tol)
    assert a[5] == b[5]   # the RandomState ends in the same state: same minibatches, same draws consumed
    assert a[6] == b[6]   # basis_hypers_ of the same structure


def _fused(basis, lik, **kw):
    fused, calls = _fit("fused", basis, lik, **kw)
    assert calls["steps"] == 12 and calls["starts"] == 3 and calls["resident"] == 0, calls
    return fused


def _resident(basis, lik, **kw):
    res, calls = _fit("resident", basis, lik, **kw)
    assert calls["resident"] == 12 and calls["steps"] == 0 and calls["starts"] == 0, calls
    return res


def _host(basis, lik, **kw):
    host, calls = _fit("host", basis, lik, **kw)
    assert calls["resident"] == 0 and calls["steps"] == 0 and calls["starts"] == 0, calls
    return host


def test_one_component_on_twelve_columns_fused_equals_the_other_two():
    """Xdim = 12, FastFoodGM(nbases=16) alone: the chain's mixture mode serves the other two loops"""
    fused = _fused("gm", "poisson")
    assert fused[4].shape == (24,)
    _same(fused, _host("gm", "poisson"), FIT_TOL, "gm d=12 fused vs host")
    _same(fused, _resident("gm", "poisson"), FIT_TOL, "gm d=12 fused vs step-per-call")


def test_a_spectral_mixture_on_three_columns_runs_on_both_device_loops():
    """Xdim = 3, Linear + FastFoodGM(nbases=8) + FastFoodGM(nbases=8) + RandomRBF, Gaussian (the variance sits in front of the
    means in z): no device loop takes this fit without the opt-in; with it the fused loop does, and -- `_fused_sgd = False` -- the
    step-per-call loop"""
    fused = _fused("cat", "gaussian", d=3)
    assert fused[4].shape == (3 + 3 + 3 + 3 + 1,) and fused[2].shape == (4,)
    _same(fused, _host("cat", "gaussian", d=3), FIT_TOL, "cat d=3 fused vs host")
    _same(fused, _resident("cat", "gaussian", d=3), FIT_TOL, "cat d=3 fused vs step-per-call")


def test_one_input_column_keeps_the_reference_s_structure_of_basis_hypers():
    fused = _fused("gm", "poisson", d=1)
    host = _host("gm", "poisson", d=1)
    assert fused[4].shape == (2,)
    _same(fused, host, FIT_TOL, "gm d=1 fused vs host")


# ---- T4: reproducibility and routing -------------------------------------------------------------------------------------

def test_launch_blocks_and_reruns_are_bit_identical():
    one, c1 = _fit("fused", "cat", "gaussian", d=3)
    cut, c2 = _fit("fused", "cat", "gaussian", d=3, block=7)
    again, _ = _fit("fused", "cat", "gaussian", d=3, block=7)
    assert c1["run"] == 1 and c2["run"] == 2 and c2["steps"] == 12
    for u, v, w in zip(one[:5], cut[:5], again[:5]):
        assert np.array_equal(u, v) and np.array_equal(v, w)
    assert one[5] == cut[5] == again[5]


def test_device_sampler_fused_equals_the_step_per_call_loop():
    """sampler="device": both device loops see the kernel generator's draws (no host loop has them)"""
    for basis, lik, d in (("gm", "poisson", 12), ("cat", "gaussian", 3)):
        fused = _fused(basis, lik, d=d, sampler="device")
        _same(fused, _resident(basis, lik, d=d, sampler="device"), FIT_TOL, "%s d=%d device sampler" % (basis, d))


def test_device_group_with_unsplittable_minibatches_runs_the_fused_loop_on_member_0():
    one = _fused("cat", "gaussian", d=3)
    many = _fused("cat", "gaussian", d=3, devices=[0, 0])
    for u, v in zip(one[:5], many[:5]):
        assert np.array_equal(u, v)
    assert one[5] == many[5]


def test_shapes_outside_the_range_keep_the_step_per_call_loop():
    """batch 300: M F = 300 x 64 > 8192 -- rr_glm_svi_supported_gm declines; the fit runs rr_glm_sgd_step as under
    fused_bases="all" (1e-8: the project's bound between two runs of that loop)"""
    from revrand_amd import _hip
    assert _hip.svi_supported_gm(64, 4, 10, 10, 1, 12, 24, 12 * 16)
    assert not _hip.svi_supported_gm(64, 4, 10, 300, 1, 12, 24, 12 * 16)
    assert not _hip.svi_supported_gm(64, 4, 10, 10, 1, 12, 24, 1 << 22)   # tables far beyond one CU's LDS
    on, calls = _fit("fused", "gm", "poisson", batch=300, maxiter=6)
    assert calls["steps"] == 0 and calls["starts"] == 0 and calls["resident"] == 6, calls
    off, calls = _fit("fused", "gm", "poisson", batch=300, maxiter=6, fused_bases="all")
    assert calls["steps"] == 0 and calls["resident"] == 6, calls
    _same(on, off, 1e-8, "gm d=12 batch 300 routed to the step-per-call loop")


def test_without_the_opt_in_three_columns_run_no_device_loop():
    out, calls = _fit("fused", "cat", "gaussian", d=3, fused_bases="all")
    assert calls == {"run": 0, "steps": 0, "starts": 0, "resident": 0}, calls
    assert np.all(np.isfinite(out[0]))


def test_create_gm_refuses_invalid_children_with_a_message_and_the_old_entry_points_still_refuse():
    from revrand_amd import _hip
    rs = np.random.RandomState(0)
    d, n, K, N = 3, 4, 2, 40
    dev = _hip.get_device()
    V = np.ascontiguousarray(rs.randn(d, n))
    rff = _hip.RffHandle(V)
    other = _hip.get_upload_device(dev.index)   # a second context of the same GPU
    with _hip.device_scope(other):
        rff_other = _hip.RffHandle(V)
    X, y = rs.randn(N, d), rs.randn(N)

    def make(child, F, n_ls, **how):
        np_ = 2 * F * K + 1 + n_ls
        return _Svi([child + (X,)], y, K, 4, 8, 3, 0, np.ones(np_), "Adam", [1e-2, 0.9, 0.99, 1e-8], 5, N / 8.0, **how)
    with pytest.raises(_hip.HipError, match=r"child 0.*n_ls"):
        make(("gm", rff, d), 4 * n, d)                         # n_ls != 2 d
    with pytest.raises(_hip.HipError, match=r"child 0.*context"):
        make(("gm", rff_other, 2 * d), 4 * n, 2 * d)           # a handle of another context
    with pytest.raises(_hip.HipError, match="RR_SGD_CHILD_GM"):
        make(("gm", rff, 2 * d), 4 * n, 2 * d, all_children=True)
    with pytest.raises(_hip.HipError, match="RR_SGD_CHILD_GM"):
        make(("gm", rff, 2 * d), 4 * n, 2 * d, all_children=False)
    make(("gm", rff, 2 * d), 4 * n, 2 * d).close()            # valid


def test_wide_components_route_under_the_opt_in_as_without_it():
    """The chain's mixture mode serves block sizes 16 .. 256; the dense child is for the sizes BELOW only: Xdim = 3 gets it under
    the opt-in (no child without), Xdim = 12 the chain child either way.  Xdim = 300 (d2 = 512) has no FastFood handle at all
    (rr_fastfood_create refuses d2 > 256): `fit` raises the same error under "all" and under "all+gm"."""
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    from revrand_amd import _hip
    rs = np.random.RandomState(0)
    X = rs.randn(40, 12)
    for d, dense in ((3, True), (12, False)):
        for kw, want in (({}, d > 8), ({"dense_gm": True}, True)):
            feats = bs.MinibatchFeatures(bs.FastFoodGM(nbases=8, Xdim=d, random_state=1))
            assert feats.make_resident(X[:, :d], "all", **kw) is want
            if want:
                assert [k.dense for k in feats._kids] == [dense and bool(kw)]
                for k in feats._kids:
                    k.release()
    X, y = rs.randn(40, 300), rs.randn(40)
    msgs = []
    for fused_bases in ("all", "all+gm"):
        glm = GLM(lk.Gaussian(), bs.FastFoodGM(nbases=8, Xdim=300, random_state=1), K=2, nsamples=4, batch_size=10, maxiter=2,
                  nstarts=1, random_state=1, resident_bases="all", fused_bases=fused_bases)
        with pytest.raises(_hip.HipError, match="256") as e:
            glm.fit(X, y)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
