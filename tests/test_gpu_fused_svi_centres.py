"""RadialBasis, SigmoidalBasis and PolynomialBasis children in the many-steps-per-launch kernel of small minibatches
(rr_glm_svi_create_all, rr_svi.hip; ``GeneralizedLinearModel(resident_bases="all", fused_bases="all")``).

* T1: one plain SGD step against the reference's recorded gradient (tests/golden/centres.npz glm_*, glm.py:205-294 with
  basis_functions.py:616-815);
* T2: every new kind at once -- linear | sigmoid (isotropic, on two columns) | polynomial | radial (ARD) with a Gaussian
  likelihood -- against the float64 oracle (oracle.glm_elbo on tests/centres_cases.py's restatement of the bases): one step,
  four Adam steps with the log trick, the batched random starts;
* T3: whole fits: fused == the step-per-call resident loop == the host loop around `_elbo`;
* T4: launches of 7 steps and reruns give the same bits, the device-group path, what stays on the step-per-call loop, refusals.

The kernel is float64 on the test's own inputs; the only float32 values it sees in T1 / T2 are the draws, which the oracle
gets rounded the same way: both sides compute the same function in float64 and the bound there is 1e-6 (the oracle's own
outputs move by < 4e-8 when its draws are rounded to float32; a wrong power of l, sign, dimension or a dropped (row, centre)
term is orders of magnitude above).  T3's bounds are the project's for exactly these comparisons (tests/test_gpu_fused_svi.py:
2e-5; tests/test_gpu_centres_loop.py's concatenation: 5e-5): the other two loops form float32 products."""
import numpy as np
import pytest

import centres_cases as cc
from conftest import normwise

pytestmark = pytest.mark.gpu

TOL = 1e-6


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
    """_hip.FusedSvi(..., all_children=True) on host arrays: uploads, runs, frees."""

    def __init__(self, children, y, K, L, M, lik, n_lik, z0, updater, par, maxiter, bmag, lower=None, upper=None, is_log=None):
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
        self.svi = _hip.FusedSvi(self.dev, kids, len(y), dy, None, None, K, L, M, lik, n_lik, z0,
                                 np.full(n, -np.inf) if lower is None else lower, np.full(n, np.inf) if upper is None else upper,
                                 np.zeros(n, dtype=bool) if is_log is None else is_log, _hip.UPDATER_IDS[updater], par, maxiter, bmag,
                                 all_children=True)

    def up(self, arr, dtype):
        b = self.dev.upload_vector(np.ascontiguousarray(arr, dtype=dtype))
        self.bufs.append(b)
        return b

    def close(self):
        self.svi.close()
        for b in self.bufs:
            b.free()


# ---- T1 ------------------------------------------------------------------------------------------------------------------

def test_one_step_against_the_reference_s_gradient(golden):
    """tests/golden/centres.npz glm_*: radial ARD + LinearBasis(onescol=True), N = 64, d = 4, 24 centres, F = 29, K = 3, L = 8,
    Bernoulli; X in float64, the minibatch all 64 rows in order (four full 16-row MFMA blocks), one plain SGD step with
    eta = 1e-3 and no log trick: (z0 - z1) / eta IS the gradient the kernel formed, objs[0] the step's -ELBO.
    Bound 1e-6: the draws are the only float32 input; rounding glm_e to float32 moves the oracle's own outputs by at most
    2.6e-8 (obj 2e-9, dm 9e-9, dC 2.6e-8, dbp 1.7e-9), and 1e-6 is 40x that floor."""
    from revrand_amd import _hip
    from revrand_amd import likelihoods as lk
    g = golden("centres")
    X, y, C, ls = g["glm_X"], g["glm_y"], g["glm_C"], g["glm_ls"]
    N, d = X.shape
    K, L, F = int(g["glm_K"]), int(g["glm_L"]), C.shape[0] + d + 1
    h = _hip.CentresHandle(C, "radial")
    z0 = np.concatenate([g["glm_m"].ravel(), g["glm_Cv"].ravel(), g["glm_regs"].ravel(), ls.ravel()])
    eta = 1e-3
    run = _Svi([("centres", h, d, X), ("linear", d, True, X)], y, K, L, N, lk.RR_LIK_BERNOULLI, 0, z0, "SGDUpdater", [eta], 1,
               float(g["glm_B"]))
    try:
        run.svi.run(1, run.up(np.arange(N), np.int32), run.up(g["glm_e"].reshape(K * L, F), np.float32))
        z1, objs, _ = run.svi.read()
    finally:
        run.close()
    grad = (z0 - z1) / eta
    fk = F * K
    got = (grad[:fk].reshape(F, K), grad[fk:2 * fk].reshape(F, K), grad[2 * fk:2 * fk + 2], grad[2 * fk + 2:])
    e = (abs(objs[0] - g["glm_obj"]) / abs(g["glm_obj"]), normwise(got[0], g["glm_ndm"]), normwise(got[1], g["glm_ndC"]),
         normwise(got[2], g["glm_dL"]), normwise(got[3], g["glm_dbp"]))
    print("fused step vs reference: obj %.2e dm %.2e dC %.2e dL %.2e dbp %.2e" % e)
    assert got[3].shape == (d,)
    assert all(v < TOL for v in e), e


# ---- T2 ------------------------------------------------------------------------------------------------------------------

class _Mixed(object):
    """Linear(onescol) | Sigmoid, isotropic, 17 centres on columns [0, 2] | Poly(order 3, no bias) | Radial, ARD, d = 9, 21
    centres; Gaussian; K = 3, L = 20, N = 80, minibatches of 20 rows (B = 4).  Widths [10, 17, 27, 21]: F = 75 (odd), M dsum =
    20 x 29 = 580, n_ls = 1 + 9 = 10 (the one-wave-per-length-scale loop takes a second turn), L and M one full 16-block plus a
    partial one, no centre child first or aligned; z = [m | C | 4 regularisers | variance | sigmoid l | radial l (9)].  Centres
    are rows of X and every minibatch holds rows 0-5: zero distances occur in both centre children."""

    N, d, K, L, M, F = 80, 9, 3, 20, 20, 75

    def __init__(self):
        rs = np.random.RandomState(7)
        self.X = rs.randn(self.N, self.d)
        self.y = np.sin(self.X[:, 0]) + 0.3 * self.X[:, 3] + 0.1 * rs.randn(self.N)
        self.ind = [0, 2]
        self.Cs, self.Cr = self.X[2:19][:, self.ind].copy(), self.X[:21].copy()
        self.B = self.N / float(self.M)
        F, K = self.F, self.K
        self.slices = [slice(0, 10), slice(10, 27), slice(27, 54), slice(54, 75)]
        self.m = 0.3 * rs.randn(F, K)
        self.C = rs.gamma(2., 0.5, size=(F, K))
        self.regs = np.array([1.3, 0.8, 2.1, 0.6])
        self.var = 0.45
        self.ls_s, self.ls_r = np.array([0.9]), np.linspace(0.8, 1.4, self.d)
        self.x0 = np.concatenate([self.m.ravel(), self.C.ravel(), self.regs, [self.var], self.ls_s, self.ls_r])
        self.positive = np.concatenate([np.zeros(F * K, dtype=bool), np.ones(self.x0.size - F * K, dtype=bool)])
        # minibatches: rows 0-5 in every one, the rest drawn without repetition; draws rounded to float32 ONCE, for both sides
        self.idx = np.stack([np.concatenate([np.arange(6), 6 + rs.permutation(self.N - 6)[:self.M - 6]]) for _ in range(4)])
        self.idx = np.stack([i[rs.permutation(self.M)] for i in self.idx]).astype(np.int32)
        self.e = rs.randn(4, K, self.L, F).astype(np.float32)

    def handles(self):
        from revrand_amd import _hip
        return _hip.CentresHandle(self.Cs, "sigmoid"), _hip.CentresHandle(self.Cr, "radial", compute="f64")   # (either compute dtype)

    def children(self, hs, hr):
        return [("linear", self.d, True, self.X), ("centres", hs, 1, self.X[:, self.ind]), ("poly", self.d, False, 3, self.X),
                ("centres", hr, self.d, self.X)]

    def elbo(self, x, idx, e):
        """oracle.glm_elbo at the flat x on rows idx with draws e (K, L, F): (-ELBO, gradient in x's layout)"""
        orc = _oracle()
        F, K, d = self.F, self.K, self.d
        m, C = x[:F * K].reshape(F, K), x[F * K:2 * F * K].reshape(F, K)
        regs, var = x[2 * F * K:2 * F * K + 4], x[2 * F * K + 4]
        ls_s, ls_r = x[2 * F * K + 5:2 * F * K + 6], x[2 * F * K + 6:]
        Xb, yb = self.X[idx], self.y[idx]
        Phi = np.hstack([orc.linear_transform(Xb, True), cc.sigmoid_transform(Xb[:, self.ind], self.Cs, ls_s),
                         cc.poly_transform(Xb, 3, False), cc.radial_transform(Xb, self.Cr, ls_r)])
        assert Phi.shape == (len(idx), F)

        def slab(block, sl):
            out = np.zeros_like(Phi)
            out[:, sl] = block
            return out
        dPhis = [slab(cc.sigmoid_grad(Xb[:, self.ind], self.Cs, ls_s), self.slices[1])]
        dr = cc.radial_grad(Xb, self.Cr, ls_r)
        dPhis += [slab(dr[:, :, i], self.slices[3]) for i in range(d)]
        rd = np.concatenate([np.full(s.stop - s.start, r) for s, r in zip(self.slices, regs)])
        obj, (ndm, ndC, dL, dlp, dbp) = orc.glm_elbo(m, C, rd, self.slices, "gaussian", [var], (), Phi, dPhis, yb,
                                                     np.asarray(e, dtype=np.float64), self.B)
        return obj, np.concatenate([ndm.ravel(), ndC.ravel(), np.ravel(dL), np.ravel(dlp), np.ravel(dbp)])

    def blocks(self, v):
        fk = self.F * self.K
        return v[:fk], v[fk:2 * fk], v[2 * fk:2 * fk + 4], v[2 * fk + 4:2 * fk + 5], v[2 * fk + 5:]


@pytest.fixture(scope="module")
def mixed():
    return _Mixed()


def test_mixed_case_has_zero_distances_and_finite_oracle_values(mixed):
    c = mixed
    assert [s.stop - s.start for s in c.slices] == [10, 17, 27, 21] and c.F % 2 == 1 and c.M * (9 + 2 + 9 + 9) == 580
    for idx in c.idx:
        assert set(range(6)) <= set(idx.tolist()) and len(set(idx.tolist())) == c.M
        Xb = c.X[idx]
        assert (np.abs(Xb[:, None, :] - c.Cr[None]).sum(axis=2) == 0).sum() >= 6          # rows 0-5 sit on radial centres
        assert (np.abs(Xb[:, None, c.ind] - c.Cs[None]).sum(axis=2) == 0).sum() >= 4      # rows 2-5 on sigmoid centres
    obj, grad = c.elbo(c.x0, c.idx[0], c.e[0])
    assert np.isfinite(obj) and np.all(np.isfinite(grad)) and np.all(grad[-10:] != 0)


def test_mixed_children_one_step_against_the_oracle(mixed):
    """(a) one plain SGD step: all five gradient blocks -- the ten length-scale gradients among them -- and the objective"""
    from revrand_amd import likelihoods as lk
    c = mixed
    hs, hr = c.handles()
    eta = 1e-4
    run = _Svi(c.children(hs, hr), c.y, c.K, c.L, c.M, lk.RR_LIK_GAUSSIAN, 1, c.x0, "SGDUpdater", [eta], 1, c.B)
    try:
        run.svi.run(1, run.up(c.idx[0], np.int32), run.up(c.e[0].reshape(c.K * c.L, c.F), np.float32))
        z1, objs, norms = run.svi.read()
    finally:
        run.close()
    obj, ref = c.elbo(c.x0, c.idx[0], c.e[0])
    got = (c.x0 - z1) / eta
    # (z0 - z1) / eta cancels: |z| ~ 1 leaves 2e-16 / eta = 2e-12 absolute on gradients of magnitude >= 1e-2 -- far below 1e-6)
    e = (abs(objs[0] - obj) / abs(obj),) + tuple(normwise(u, v) for u, v in zip(c.blocks(got), c.blocks(ref)))
    print("mixed children, one step vs oracle: obj %.2e dm %.2e dC %.2e dL %.2e dvar %.2e dls %.2e" % e)
    print("   length-scale gradients (oracle):", np.array2string(c.blocks(ref)[4], precision=3))
    assert abs(norms[0] - np.linalg.norm(ref)) < TOL * np.linalg.norm(ref)
    assert all(v < TOL for v in e), e


def test_mixed_children_four_adam_steps_with_the_log_trick(mixed):
    """(b) four Adam steps over four different minibatches with every positive coordinate in log space, replayed with
    oracle.glm_elbo, the chain rule of the log trick (decorators.py:329-408), oracle.sgd_update and the clip (sgd.py:404-420):
    the per-slot 1 / l^6 and 1 / l^2 behind the chain rule, the parity buffers, the prefetched gather of the next step."""
    from revrand_amd import likelihoods as lk
    orc = _oracle()
    c = mixed
    pos = c.positive
    z0 = np.where(pos, np.log(np.where(pos, c.x0, 1.0)), c.x0)
    lower = np.where(pos, np.log(1e-14), -np.inf)
    upper = np.full(z0.size, np.inf)
    hs, hr = c.handles()
    run = _Svi(c.children(hs, hr), c.y, c.K, c.L, c.M, lk.RR_LIK_GAUSSIAN, 1, z0, "Adam", [0.01, 0.9, 0.99, 1e-8], 4, c.B,
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
    print("mixed children, four Adam steps vs oracle: m %.2e logC %.2e log reg %.2e log var %.2e log ls %.2e objs %.2e" % e)
    assert np.abs(z4 - z0).max() > 0.02   # (the steps moved the parameters)
    assert all(v < TOL for v in e), e


def test_mixed_children_random_starts_against_the_oracle(mixed):
    """(c) FusedSvi.starts on three candidates, each on its own minibatch with its own draws: oracle.glm_elbo's objective"""
    from revrand_amd import likelihoods as lk
    c = mixed
    rs = np.random.RandomState(3)
    cands = np.stack([np.where(c.positive, c.x0 * np.exp(0.2 * rs.randn(c.x0.size)), c.x0 + 0.1 * rs.randn(c.x0.size)) for _ in range(3)])
    hs, hr = c.handles()
    run = _Svi(c.children(hs, hr), c.y, c.K, c.L, c.M, lk.RR_LIK_GAUSSIAN, 1, c.x0, "Adam", [0.01, 0.9, 0.99, 1e-8], 1, c.B)
    try:
        got = run.svi.starts(run.up(c.idx[1:4], np.int32), cands, run.up(c.e[1:4].reshape(3, c.K * c.L, c.F), np.float32))
    finally:
        run.close()
    ref = np.array([c.elbo(cands[i], c.idx[1 + i], c.e[1 + i])[0] for i in range(3)])
    e = np.abs(got - ref) / np.abs(ref)
    print("mixed children, random starts vs oracle:", e)
    assert len(set(np.round(ref, 6))) == 3 and np.all(e < TOL), (got, ref)


# ---- T3: fits ------------------------------------------------------------------------------------------------------------

def _data(lik, N=500, d=4, seed=4):
    rs = np.random.RandomState(seed)
    X = rs.randn(N, d)
    f = 0.5 * np.sin(X[:, 0]) + 0.2 * X[:, 2]
    if lik == "poisson":
        return X, rs.poisson(np.exp(f)).astype(float), ()
    if lik == "binomial":
        n = rs.randint(5, 30, size=N).astype(float)
        return X, rs.binomial(n.astype(int), 1 / (1 + np.exp(-3 * f))).astype(float), (n,)
    return X, f + 0.1 * rs.randn(N), ()


def _basis(name, X):
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    d = X.shape[1]
    if name == "cat":   # linear | radial ARD | RandomRBF | poly | sigmoid iso on apply_ind=[0, 2]
        from test_gpu_centres_loop import _cat
        return _cat(X)()
    if name == "cat_gm":   # a spectral-mixture child: the step-per-call loop's alone (its chain kernel serves Xdim > 8: d = 12)
        return bs.RadialBasis(centres=X[:21].copy(), lenscale=Parameter(np.ones(d), Positive())) \
            + bs.FastFoodGM(nbases=16, Xdim=d, random_state=2)
    if name == "poly":
        return bs.PolynomialBasis(order=2)
    kind, ls = name.split("_")
    cls = bs.RadialBasis if kind == "radial" else bs.SigmoidalBasis
    M = 65 if ls.endswith("65") else 21
    lenscale = {"ard": lambda: Parameter(np.ones(d), Positive()), "iso": lambda: Parameter(1.0, Positive()),
                "bound": lambda: Parameter(np.ones(d), Bound(0.995, 1.004)), "ard65": lambda: Parameter(np.ones(d), Positive())}[ls]()
    return cls(centres=X[:M].copy(), lenscale=lenscale)


def _fit(loop, basis, lik="poisson", updater=None, sampler="host", maxiter=25, K=4, L=10, batch=10, nstarts=3, block=None,
         devices=None, fused_bases="all", d=4):
    bs, lk, opt, Bound, Parameter, Positive, GLM = _imports()
    from revrand_amd import _hip
    from revrand_amd import glm as glm_mod
    X, y, largs = _data(lik, d=d)
    like = {"poisson": lk.Poisson, "binomial": lk.Binomial, "gaussian": lk.Gaussian}[lik]()
    glm = GLM(like, _basis(basis, X), K=K, nsamples=L, batch_size=batch, maxiter=maxiter, nstarts=nstarts, random_state=11,
              updater=updater() if updater is not None else None, sampler=sampler, resident_bases="all", fused_bases=fused_bases,
              devices=devices)
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
    return (glm.weights_.copy(), glm.covariance_.copy(), flat(glm.regularizer_), flat(glm.like_hypers_), flat(glm.basis_hypers_),
            glm.random_.randn()), calls


def _same(a, b, tol, what=""):
    worst = max([normwise(u, v) for u, v in zip(a[:5], b[:5]) if u.size])
    print("%s: worst block %.3e (bound %.0e)" % (what, worst, tol))
    for u, v in zip(a[:5], b[:5]):
        assert u.shape == v.shape
        if u.size:
            assert np.all(np.isfinite(u)) and normwise(u, v) < tol, (normwise(u, v), tol)
    assert a[5] == b[5]   # the RandomState ends in the same state: same minibatches, same draws consumed


def _three_loops(basis, lik, tol, n_ls, **kw):
    maxiter = kw.get("maxiter", 25)
    fused, calls = _fit("fused", basis, lik, **kw)
    assert calls["steps"] == maxiter and calls["starts"] == 3 and calls["resident"] == 0, calls
    res, calls = _fit("resident", basis, lik, **kw)
    assert calls["resident"] == maxiter and calls["steps"] == 0 and calls["starts"] == 0, calls
    host, calls = _fit("host", basis, lik, **kw)
    assert calls["resident"] == 0 and calls["steps"] == 0 and calls["starts"] == 0, calls
    assert fused[4].shape == (n_ls,)
    _same(fused, host, tol, "%s %s fused vs host" % (basis, lik))
    _same(fused, res, tol, "%s %s fused vs step-per-call" % (basis, lik))
    return fused


@pytest.mark.parametrize("basis,lik,n_ls", [("radial_ard", "poisson", 4), ("radial_iso", "gaussian", 1), ("sigmoid_ard", "gaussian", 4),
                                            ("sigmoid_iso", "poisson", 1)])
def test_centre_children_fused_equals_the_other_two(basis, lik, n_ls):
    """21 centres X[:21], batch 10, K = 4, L = 10, 25 Adam steps, 3 random starts; the Gaussian's variance sits in front of
    the length scales in z (read-back, set_start and basis_hypers_ go through that offset)."""
    _three_loops(basis, lik, 2e-5, n_ls)


def test_polynomial_basis_alone_has_no_length_scale():
    fused = _three_loops("poly", "gaussian", 2e-5, 0)
    assert fused[0].shape == (9, 4)


def test_concatenation_with_an_rff_and_two_centre_children():
    """tests/test_gpu_centres_loop.py's concatenation on four input columns: five regularisers, 4 + 1 + 1 length scales
    (radial ARD, RandomRBF, sigmoid isotropic on apply_ind=[0, 2]) -- a random Fourier child's slot between two centre children's"""
    fused = _three_loops("cat", "binomial", 5e-5, 6)
    assert fused[2].shape == (5,)


def test_a_plain_bound_on_the_radial_length_scales_is_hit():
    """Bound(0.995, 1.004) without the log trick: the truncation and the clip of sgd.py:404-420 behind the 1 / l^6"""
    fused = _three_loops("radial_bound", "poisson", 2e-5, 4)
    rl = fused[4]
    assert np.all(rl >= 0.995) and np.all(rl <= 1.004) and (np.any(rl == 0.995) or np.any(rl == 1.004))


@pytest.mark.parametrize("name", ["SGDUpdater", "AdaDelta", "AdaGrad", "Momentum", "Adam"])
def test_every_updater_on_the_radial_ard_basis(name):
    opt = _imports()[2]
    mk = {"SGDUpdater": lambda: opt.SGDUpdater(eta=1e-4), "Momentum": lambda: opt.Momentum(rho=0.5, eta=1e-4),
          "AdaGrad": lambda: opt.AdaGrad(eta=1e-2)}.get(name, getattr(opt, name))
    _three_loops("radial_ard", "poisson", 2e-5, 4, updater=mk)


def test_device_sampler_fused_equals_the_step_per_call_loop():
    """sampler="device": both device loops see the kernel generator's draws (no host loop has them)"""
    for basis, lik, tol in (("radial_ard", "poisson", 2e-5), ("cat", "gaussian", 5e-5)):
        fused, calls = _fit("fused", basis, lik, sampler="device")
        assert calls["steps"] == 25 and calls["starts"] == 3 and calls["resident"] == 0
        res, calls = _fit("resident", basis, lik, sampler="device")
        assert calls["resident"] == 25 and calls["steps"] == 0
        _same(fused, res, tol, "%s %s device sampler" % (basis, lik))


# ---- T4: reproducibility and routing -------------------------------------------------------------------------------------

def test_launch_blocks_and_reruns_are_bit_identical():
    one, c1 = _fit("fused", "radial_ard", "poisson")
    cut, c2 = _fit("fused", "radial_ard", "poisson", block=7)
    again, _ = _fit("fused", "radial_ard", "poisson", block=7)
    assert c1["run"] == 1 and c2["run"] == 4 and c2["steps"] == 25
    for u, v, w in zip(one[:5], cut[:5], again[:5]):
        assert np.array_equal(u, v) and np.array_equal(v, w)
    assert one[5] == cut[5] == again[5]


def test_device_group_with_unsplittable_minibatches_runs_the_fused_loop_on_member_0():
    one, c1 = _fit("fused", "radial_ard", "poisson")
    many, c2 = _fit("fused", "radial_ard", "poisson", devices=[0, 0])
    assert c1["steps"] == 25 and c2["steps"] == 25 and c2["starts"] == 3 and c2["resident"] == 0
    for u, v in zip(one[:5], many[:5]):
        assert np.array_equal(u, v)
    assert one[5] == many[5]


def test_shapes_outside_the_range_and_gm_children_keep_the_step_per_call_loop():
    """batch 300 x 65 centres: M F = 19500 > 8192 -- rr_glm_svi_supported_all declines; a FastFoodGM child is not taken.
    Both run rr_glm_sgd_step as under fused_bases="fourier" (1e-8: the project's bound between two runs of that loop,
    tests/test_gpu_centres_loop.py T5)."""
    from revrand_amd import _hip
    assert _hip.svi_supported_all(21, 4, 10, 10, 1, 4, 4, 4 * 21)
    assert not _hip.svi_supported_all(65, 4, 10, 300, 1, 4, 4, 4 * 65)
    assert not _hip.svi_supported_all(21, 4, 10, 10, 1, 4, 4, 1 << 22)   # tables far beyond one CU's LDS
    for basis, kw in (("radial_ard65", dict(batch=300, maxiter=6)), ("cat_gm", dict(maxiter=6, d=12))):
        on, calls = _fit("fused", basis, "poisson", **kw)
        assert calls["steps"] == 0 and calls["starts"] == 0 and calls["resident"] == 6, calls
        off, calls = _fit("fused", basis, "poisson", fused_bases="fourier", **kw)
        assert calls["steps"] == 0 and calls["resident"] == 6, calls
        _same(on, off, 1e-8, basis + " routed to the step-per-call loop")


def test_create_all_refuses_invalid_children_with_a_message():
    from revrand_amd import _hip
    rs = np.random.RandomState(0)
    d, M, K, N = 3, 5, 2, 40
    C = rs.randn(M, d)
    dev = _hip.get_device()
    h32 = _hip.CentresHandle(C, "radial")
    other = _hip.get_upload_device(dev.index)   # a second context of the same GPU
    with _hip.device_scope(other):
        h_other = _hip.CentresHandle(C, "radial")
    rff = _hip.RffHandle(np.ascontiguousarray(rs.randn(d, 4)))
    dX = dev.upload_matrix(np.ascontiguousarray(rs.randn(N, d), dtype=np.float64))
    dy = dev.upload_vector(rs.randn(N), np.float64)

    def make(child, F, n_ls):
        np_ = 2 * F * K + 1 + n_ls
        return _hip.FusedSvi(dev, [child], N, dy, None, None, K, 4, 8, 3, 0, np.ones(np_), np.full(np_, -np.inf), np.full(np_, np.inf),
                             np.zeros(np_, dtype=bool), _hip.UPDATER_IDS["Adam"], [1e-2, 0.9, 0.99, 1e-8], 5, N / 8.0, all_children=True)
    try:
        for child, F, n_ls, word in ((("centres", h32, 2, dX), M, 2, "centres basis"), (("centres", h_other, d, dX), M, d, "centres basis"),
                                     (("poly", 0, True, 2, dX), 1, 0, "polynomial"), (("poly", d, True, -1, dX), 1, 0, "polynomial"),
                                     (("poly", d, False, 0, dX), 0, 0, "polynomial")):
            with pytest.raises(_hip.HipError, match=word):
                make(child, F, n_ls)
        with pytest.raises(_hip.HipError, match="RR_SGD_CHILD_GM"):
            make(("gm", rff, 2 * d, dX), 16, 2 * d)
        make(("centres", h32, d, dX), M, d).close()                  # valid
        make(("poly", d, True, 0, dX), 1, 0).close()                  # valid: a bias column alone
    finally:
        dX.free()
        dy.free()
