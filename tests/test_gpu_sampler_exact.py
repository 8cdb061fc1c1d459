"""The device sampler (sampler="device") draw by draw: every normal the GPU generates, recovered bit for bit through the
identity set-up of tests/sampler_cases.py and held to the host model of the generator there -- which function of (seed, step,
weight sample, feature) a draw is -- in every kernel that holds a copy of the generator and under every key derivation:

  A  rr_featmat_glm_step_sampled (rr_glm_draw_kernel, rr_elbo.hip), both likelihood routes, F on and across a 256-column pad
     block, a seed beyond 2^31, K L factored three ways, after a wider step has grown the scratch;
  B  ResidentSgd.step (the same kernel launched by rr_glm_sgd_step), one and two streams, one step and three;
  C  FusedSvi.run (rr_svi_draw, rr_svi_common.h, in rr_svi.hip's svi_draws: step 0 and the prefetch of step t + 1), F even and odd, launches cut 3 and 2 + 1;
  D  FusedSvi.starts (candidate c on step key0 + c);
  E  the keys glm.py hands down over a fit: 0 .. nstarts - 1 to the starts, then consecutive, a new seed per fit.

The bound B on |e_device - e_model| (float32 __logf and hardware cosine against float64 from the same two 24-bit integers)
cannot be derived: it is 4 x the maximum MEASURED over every draw of A on an MI355X (room for compiler and ROCm drift; the
kernel is deterministic), and must not exceed 1e-5 -- float32 values in the tail (|e| >= 4) are 4.8e-7 apart, a wrong draw is
O(1) away.
    measured max |e_device - e_model| over A: 4.655e-07      B = 1.87e-06      (docs/KERNELS.md 3.46)

B, C and D compare with A's recovered draws: bit for bit where the arithmetic is exact, through a float64 replay elsewhere."""
import numpy as np
import pytest

import revrand_oracle as orc
import sampler_cases as sc
from conftest import normwise
from test_gpu_glm_routes import _Mode, _linear_features

pytestmark = pytest.mark.gpu

MEASURED_MAX = 4.655e-07
B = 1.87e-06
GAUSS = 2          # RR_LIK_GAUSSIAN
ETA, BMAG = 2.0 ** -4, 2.0


def _say(name, value):
    print("MEASURED %s %.3e" % (name, value))
    return value


def test_the_bound_is_four_times_the_measurement_and_under_its_cap():
    assert 4 * MEASURED_MAX <= B <= 4.1 * MEASURED_MAX and B <= sc.B_CAP


# ---- A: the step ---------------------------------------------------------------------------------------------------------
def _sampled(f, F, K, L, seed, step):
    """(Edm, EdC, C), (F, K) each, of one identity step on MinibatchFeatures f"""
    X, y, m, C = sc.identity_step(F, K)
    f.assemble(X, [])
    Edm, EdC, _, _ = f.glm_step_sampled(y, None, GAUSS, 1.0, m, C, K, L, seed, step)
    assert Edm.shape == EdC.shape == (F, K)
    return np.array(Edm), np.array(EdC), C


def _recover_on(f, F, seed, step):
    e = sc.draws_from_step(*_sampled(f, F, sc.STEP_KL, 1, seed, step))
    assert e.shape == (sc.STEP_KL, F) and np.array_equal(e, e.astype(np.float32).astype(np.float64))
    return e


_DRAWS = {}


def device_draws(F, seed, step):
    """The K L = 64 draws of (seed, step) at F features as rr_glm_draw_kernel makes them, (64, F) float64 holding float32
    values; computed once per (F, seed, step) and shared (read only)."""
    if (F, seed, step) not in _DRAWS:
        f = _linear_features()
        try:
            e = _recover_on(f, F, seed, step)
        finally:
            f.release()
        e.setflags(write=False)
        _DRAWS[(F, seed, step)] = e
    return _DRAWS[(F, seed, step)]


def _assert_rel(got, want, tol, what):
    """elementwise |got - want| <= tol |want|"""
    bad = ~(np.abs(got - want) <= tol * np.abs(want))
    assert not bad.any(), "%s: %d of %d outside %g relative, worst |diff| %g" % (what, int(bad.sum()), bad.size, tol,
                                                                               np.abs(got - want)[bad].max())


@pytest.mark.parametrize("mode", ["0", "force"])
@pytest.mark.parametrize("F", sc.STEP_F)
def test_step_draws_are_the_models(F, mode):
    """K = 64, L = 1, C[:, k] = 4^-(k mod 3) (pins k = kl / L): every recovered draw within B of model_draws, for two seeds
    (one >= 2^31) x steps 0 and 7.  Then K L = 64 as (8, 8) and (4, 16): Edm and EdC are the sums over l of the draws recovered
    with K = 64 -- a draw depends on kl, not on how K L factors -- in the kernel's order, so 1e-15 relative per element.  Last,
    the K L = 64 case once more after a K L = 512 step has widened the scratch (its sample width only grows)."""
    worst = 0.0
    f = _linear_features()
    try:
        with _Mode(mode):
            first = None
            for seed in sc.STEP_SEEDS:
                for step in sc.STEP_STEPS:
                    e = _recover_on(f, F, seed, step)
                    first = (seed, step, e) if first is None else first
                    assert np.array_equal(e, device_draws(F, seed, step)), "the draws depend on the likelihood route"
                    model = sc.model_draws(seed, step, sc.STEP_KL, 1, F)
                    d = np.abs(e - model)
                    kl, j = np.unravel_index(np.argmax(d), d.shape)
                    worst = max(worst, _say("max |e_device - e_model| F=%d RR_GLM_FUSE_LIK=%s seed=%d step=%d" % (F, mode, seed, step),
                                            float(d.max())))
                    assert d.max() <= B, "F=%d seed=%d step=%d: draw (kl=%d, f=%d) device=%r model=%r" % (
                        F, seed, step, kl, j, e[kl, j], model[kl, j])
                    for K, L in sc.STEP_FACTORINGS:
                        Edm, EdC, C = _sampled(f, F, K, L, seed, step)
                        want_m, want_C = sc.reduced_from_draws(e, K, L, C)
                        _assert_rel(Edm, want_m, 1e-15, "Edm (K, L) = %s seed=%d step=%d" % ((K, L), seed, step))
                        _assert_rel(EdC, want_C, 1e-15, "EdC (K, L) = %s seed=%d step=%d" % ((K, L), seed, step))
            seed, step, e = first
            _sampled(f, F, sc.STEP_WIDE[0], sc.STEP_WIDE[1], seed, step)
            assert np.array_equal(_recover_on(f, F, seed, step), e), "K L = 64 after K L = 512"
    finally:
        f.release()
    _say("max |e_device - e_model| F=%d RR_GLM_FUSE_LIK=%s" % (F, mode), worst)


def test_model_counters_are_not_the_padded_ones():
    """What the cases above would let through if the model's own F were wrong: at F = 300 the model with the row length in HBM
    (512) or the next multiple of 256 differs from the model with F from the second row on."""
    a = sc.model_draws(11, 0, 2, 1, 300)
    assert np.array_equal(sc.model_draws(11, 0, 2, 1, 512)[0, :300], a[0])
    assert np.abs(sc.model_draws(11, 0, 2, 1, 512)[1, :300] - a[1]).max() > 1.0


# ---- B: the resident step --------------------------------------------------------------------------------------------------
def _resident(F, K, keys, seed, freeze, monkeypatch, overlap):
    """z after ResidentSgd steps at `keys` on the identity data: plain SGD, no log trick; freeze: every coordinate but m held
    by lower = upper = z0."""
    from revrand_amd import _hip
    monkeypatch.setenv("RR_GLM_SGD_OVERLAP", overlap)
    dev = _hip.get_device()
    z0 = sc.loop_z0(F, K)
    lower, upper = np.full(z0.size, -np.inf), np.full(z0.size, np.inf)
    if freeze:
        lower[F * K:], upper[F * K:] = z0[F * K:], z0[F * K:]
    fm = _hip.FeatureMatrix(F, F)
    dX, dy = dev.upload_matrix(np.eye(F)), dev.upload_vector(np.zeros(F), np.float32)
    sgd = None
    try:
        sgd = _hip.ResidentSgd(fm, [("linear", F, False)], K, 1, z0, lower, upper, np.zeros(z0.size, dtype=bool),
                               _hip.UPDATER_IDS["SGDUpdater"], [ETA], len(keys))
        for key in keys:
            sgd.step([dX], F, dy, None, GAUSS, 0.0, BMAG, 1, None, seed, key)
        z, objs, _ = sgd.read()
        assert len(objs) == len(keys)
    finally:
        if sgd is not None:
            sgd.close()
        dX.free()
        dy.free()
    return z


def _replay(F, K, L, draws, rows=None):
    """m after plain SGD steps on the identity data with everything but m held (C = 1, reg = 1, var = 1), in float64, step t
    on draws[t] (K L, F) and rows rows[t] of I_F (all of them by default):  m <- m - eta (-dm) with the oracle's gradient,
    (bmag (m + mean_l e) + m / reg - mixture term) / K on the rows' features -- the components' means differ from the second
    step on, and the mixture's mean term with them."""
    m, C = np.zeros((F, K)), np.ones((F, K))
    for t, e in enumerate(draws):
        X = np.eye(F) if rows is None else np.eye(F)[rows[t]]
        _, grads = orc.glm_elbo(m, C, np.ones(F), [slice(0, F)], "gaussian", [1.0], [], X, [], np.zeros(X.shape[0]),
                                np.asarray(e, dtype=float).reshape(K, L, F), BMAG)
        m = m - ETA * grads[0]
    return m


@pytest.mark.parametrize("overlap", ["0", "1"], ids=["one stream", "two streams"])
@pytest.mark.parametrize("F", sc.STEP_F)
def test_resident_step_draws_are_the_steps(F, overlap, monkeypatch):
    """K = 4, L = 1, m = 0, C = 1: the mixture's mean term is exactly 0, eta, bmag and K are powers of two, so
    z1[:F K] = -eta bmag e / K exactly: the draws are those of A for (seed, step = key), bit for bit.  Then keys 5, 6, 7 with
    only m free against the float64 replay on the single steps' draws: the step rounds w to float32, 6e-8 relative per step,
    1e-6 normwise over three; a wrong key moves the result by O(1)."""
    K, seed = sc.LOOP_K, sc.LOOP_SEED
    for key in sc.LOOP_KEYS:
        z = _resident(F, K, [key], seed, False, monkeypatch, overlap)
        e = (-z[:F * K] * (K / (ETA * BMAG))).reshape(F, K).T
        assert np.array_equal(e, device_draws(F, seed, key)[:K]), "key %d" % key
        assert np.abs(e - sc.model_draws(seed, key, K, 1, F)).max() <= B
    z = _resident(F, K, list(sc.LOOP_KEYS), seed, True, monkeypatch, overlap)
    want = _replay(F, K, 1, [device_draws(F, seed, key)[:K] for key in sc.LOOP_KEYS])
    assert np.array_equal(z[F * K:], sc.loop_z0(F, K)[F * K:])
    err = _say("resident three steps F=%d overlap=%s normwise" % (F, overlap), normwise(z[:F * K].reshape(F, K), want))
    assert err < 1e-6
    # (what the bound tells apart: the same replay with step 6's draws taken for step 7)
    wrong = _replay(F, K, 1, [device_draws(F, seed, key)[:K] for key in (5, 6, 6)])
    assert normwise(wrong, want) > 0.1


# ---- C, D: the fused loop ------------------------------------------------------------------------------------------------
# The fused kernel gathers a step's rows into registers, at most M dsum <= 1024 entries (SVI_GREG x SVI_THREADS, rr_svi.hip;
# dsum = F for the one linear child): all 38 rows of I_38 in one step are outside rr_glm_svi_supported.  A step here takes
# SVI_M = 19 of the F resident rows, sc.svi_rows(F, t): a feature whose row is absent gets an exactly zero data gradient, the
# others reveal their draw as before; the three row sets together cover every feature, and the replays take the same rows.
class _Fused(object):
    """FusedSvi on the identity data: one linear child, X = I_F float64 resident (N = F), y = 0, plain SGD, M = SVI_M rows
    per step: idx[t] of launch step t (or of candidate t)."""

    def __init__(self, F, K, L, z0, idx, freeze=False):
        from revrand_amd import _hip
        idx = np.asarray(idx)
        M = idx.shape[1]
        assert _hip.svi_supported(F, K, L, M, 1, F, 0)
        dev = _hip.get_device()
        lower, upper = np.full(z0.size, -np.inf), np.full(z0.size, np.inf)
        if freeze:
            lower[F * K:], upper[F * K:] = z0[F * K:], z0[F * K:]
        self.idx = idx
        self.bufs = [dev.upload_matrix(np.eye(F)), dev.upload_vector(np.zeros(F), np.float64)]
        self.svi = None
        try:
            self.svi = _hip.FusedSvi(dev, [("linear", F, False, self.bufs[0])], F, self.bufs[1], None, None, K, L, M, GAUSS, 1, z0,
                                     lower, upper, np.zeros(z0.size, dtype=bool), _hip.UPDATER_IDS["SGDUpdater"], [ETA], len(idx),
                                     BMAG)
        except Exception:
            self.close()
            raise

    def _up(self, rows):
        self.bufs.append(self.svi.dev.upload_vector(rows, np.int32))
        return self.bufs[-1]

    def run(self, cuts, seed, key0):
        """launches of cuts[0], cuts[1], ... steps from key0 on, step t of the whole run on rows idx[t]; z afterwards"""
        t = 0
        for n in cuts:
            self.svi.run(n, self._up(self.idx[t:t + n]), None, seed, key0 + t)
            t += n
        return self.svi.read()[0]

    def starts(self, cand, seed, key0):
        assert len(cand) == len(self.idx)
        return self.svi.starts(self._up(self.idx), cand, None, seed, key0)

    def close(self):
        if self.svi is not None:
            self.svi.close()
        for b in self.bufs:
            b.free()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


@pytest.mark.parametrize("F", sc.SVI_F)
def test_fused_single_step_draws_are_the_steps(F):
    """A one-step launch, K = 4, L = 1, on each of the three row sets: z1[f K + k] = -eta bmag e[k][f] / K exactly for the
    features f whose row the step took (the kernel is float64 throughout), exactly 0 for the others, and e is array_equal to
    A's draws -- svi_draws and rr_glm_draw_kernel call the same float32 expression, rr_svi_draw.  F = 38: the kernel's row length in LDS is 39."""
    K, seed = sc.LOOP_K, sc.LOOP_SEED
    seen = np.zeros(F, dtype=bool)
    for key in sc.LOOP_KEYS:
        for t in range(3):
            rows = sc.svi_rows(F, t)
            with _Fused(F, K, 1, sc.loop_z0(F, K), [rows]) as fs:
                z = fs.run([1], seed, key)
            e = (-z[:F * K] * (K / (ETA * BMAG))).reshape(F, K).T
            want = np.zeros((K, F))
            want[:, rows] = device_draws(F, seed, key)[:K, rows]
            assert np.array_equal(e, want), "key %d rows %d: the two copies of the generator differ" % (key, t)
            assert np.abs(e[:, rows] - sc.model_draws(seed, key, K, 1, F)[:, rows]).max() <= B
            seen[rows] = True
    assert seen.all()


@pytest.mark.parametrize("cuts", [(3,), (2, 1)], ids=["3", "2+1"])
@pytest.mark.parametrize("F", sc.SVI_F)
def test_fused_launch_steps_use_consecutive_keys(F, cuts):
    """Three steps from key0 = 5, in one launch and cut 2 + 1, only m free, step t on row set t: the float64 replay on the draws
    of keys 5, 6, 7 to 1e-12 normwise (a few float64 operations per step) -- the prefetch of step t + 1 inside a launch takes
    key0 + t + 1."""
    K, seed = sc.LOOP_K, sc.LOOP_SEED
    rows = [sc.svi_rows(F, t) for t in range(3)]
    with _Fused(F, K, 1, sc.loop_z0(F, K), rows, freeze=True) as fs:
        z = fs.run(cuts, seed, sc.LOOP_KEYS[0])
    want = _replay(F, K, 1, [device_draws(F, seed, key)[:K] for key in sc.LOOP_KEYS], rows)
    assert np.array_equal(z[F * K:], sc.loop_z0(F, K)[F * K:])
    err = _say("fused three steps F=%d cuts=%s normwise" % (F, cuts), normwise(z[:F * K].reshape(F, K), want))
    assert err < 1e-12
    wrong = _replay(F, K, 1, [device_draws(F, seed, key)[:K] for key in (5, 5, 6)], rows)   # the prefetch on step t's key
    assert normwise(wrong, want) > 0.1


def test_fused_samples_of_a_component_are_consecutive_rows():
    """K = 2, L = 8, one step on row set 1, F = 38, m = 0, C = 1: z1's m block is -eta bmag mean_l e / K on the rows' features
    and the C block's gradient the oracle's, with the K L = 16 draws recovered in A: to 1e-12 of the summed magnitudes (m) / of
    the gradient (C; plus the rounding of z0 - z1)."""
    F, (K, L), seed, key = sc.SVI_F[0], sc.SVI_KL, sc.LOOP_SEED, sc.LOOP_KEYS[0]
    rows = sc.svi_rows(F, 1)
    z0 = sc.loop_z0(F, K)
    with _Fused(F, K, L, z0, [rows]) as fs:
        z = fs.run([1], seed, key)
    e = device_draws(F, seed, key)[:K * L].reshape(K, L, F)
    got_m = z[:F * K].reshape(F, K)
    want_m, bound = np.zeros((F, K)), np.zeros((F, K))
    want_m[rows] = (-ETA * BMAG * e.mean(axis=1).T / K)[rows]
    bound[rows] = (1e-12 * ETA * BMAG * np.abs(e).mean(axis=1).T / K)[rows]
    assert np.all(np.abs(got_m - want_m) <= bound), np.abs(got_m - want_m).max()
    _, grads = orc.glm_elbo(np.zeros((F, K)), np.ones((F, K)), np.ones(F), [slice(0, F)], "gaussian", [1.0], [], np.eye(F)[rows],
                            [], np.zeros(len(rows)), e, BMAG)
    got_C = ((z0 - z)[F * K:2 * F * K] / ETA).reshape(F, K)
    assert np.all(np.abs(got_C - grads[1]) <= 1e-12 * np.abs(grads[1]) + 8 * 2.0 ** -53 / ETA), np.abs(got_C - grads[1]).max()
    assert np.abs(grads[1] - grads[1][0, 0]).max() > 0.1     # (the draws are in it)


def test_fused_starts_use_key0_plus_candidate():
    """Three candidates, m = 0, C[f][k] = (1 + (f + 38 k) / 64)^2 -- a weight of its own per coordinate, so a permuted counter
    changes the sum -- K = 2, L = 8, candidate c on row set c: objs[c] is the oracle's objective on the recovered draws of key
    key0 + c to 1e-12 relative, and the three differ by more than 1e-3 relative."""
    F, (K, L), seed, key0 = sc.SVI_F[0], sc.SVI_KL, sc.LOOP_SEED, sc.STARTS_KEY0
    C, reg, var = sc.starts_C(F, K), 1.5, 0.75
    cand = np.tile(sc.loop_z0(F, K, C, reg, var), (3, 1))
    rows = [sc.svi_rows(F, c) for c in range(3)]
    with _Fused(F, K, L, sc.loop_z0(F, K), rows) as fs:
        objs = fs.starts(cand, seed, key0)
    want = np.array([orc.glm_elbo(np.zeros((F, K)), C, np.full(F, reg), [slice(0, F)], "gaussian", [var], [], np.eye(F)[rows[c]], [],
                                  np.zeros(sc.SVI_M), device_draws(F, seed, key0 + c)[:K * L].reshape(K, L, F), BMAG)[0]
                     for c in range(3)])
    rel = np.abs(objs - want) / np.abs(want)
    _say("starts objective relative", rel.max())
    assert rel.max() <= 1e-12, (objs, want)
    for a in range(3):
        for b in range(a):
            assert abs(want[a] - want[b]) > 1e-3 * abs(want[a])


# ---- E: the keys over a fit ----------------------------------------------------------------------------------------------
NSTARTS, MAXITER = 3, 20


def _spied_fits(loop, monkeypatch):
    """Two fits of ONE estimator with sampler="device"; per fit the calls [(what, seed, key, count)] in order."""
    import revrand_amd.basis_functions as bs
    from revrand_amd import _hip
    from revrand_amd import glm as glm_mod
    from revrand_amd import likelihoods as lk
    calls = []
    real_run, real_starts, real_step = _hip.FusedSvi.run, _hip.FusedSvi.starts, _hip.ResidentSgd.step
    real_sampled = bs.MinibatchFeatures.glm_step_sampled

    def run(self, steps, didx, dE=None, seed=0, key0=0):
        assert dE is None
        calls.append(("run", seed, key0, steps))
        return real_run(self, steps, didx, dE, seed, key0)

    def starts(self, didx, cand, dE=None, seed=0, key0=0):
        assert dE is None
        calls.append(("starts", seed, key0, len(cand)))
        return real_starts(self, didx, cand, dE, seed, key0)

    def step(self, dXs, rows, dy, drowarg, lik, llconst, bmag, L, dE=None, seed=0, key=0, comm=None):
        assert dE is None
        calls.append(("step", seed, key, 1))
        return real_step(self, dXs, rows, dy, drowarg, lik, llconst, bmag, L, dE, seed, key, comm=comm)

    def sampled(self, y, rowarg, lik, lik_param, m, C, K, L, seed, step, objective_only=False):
        calls.append(("objective" if objective_only else "sampled", seed, step, 1))
        return real_sampled(self, y, rowarg, lik, lik_param, m, C, K, L, seed, step, objective_only)
    monkeypatch.setattr(_hip.FusedSvi, "run", run)
    monkeypatch.setattr(_hip.FusedSvi, "starts", starts)
    monkeypatch.setattr(_hip.ResidentSgd, "step", step)
    monkeypatch.setattr(bs.MinibatchFeatures, "glm_step_sampled", sampled)
    monkeypatch.setattr(glm_mod._FusedLoop, "BLOCK_STEPS", 7)
    rs = np.random.RandomState(4)
    X = rs.randn(200, 3)
    y = 0.5 * np.sin(X[:, 0]) + 0.1 * rs.randn(200)
    glm = glm_mod.GeneralizedLinearModel(lk.Gaussian(), bs.RandomRBF(nbases=6, Xdim=3, random_state=1), K=2, nsamples=4,
                                         batch_size=10, maxiter=MAXITER, nstarts=NSTARTS, random_state=11, sampler="device")
    glm._resident_sgd = True
    glm._fused_sgd = loop == "fused"
    fits = []
    for _ in range(2):
        del calls[:]
        glm.fit(X, y)
        fits.append(list(calls))
        assert glm._dev_step == NSTARTS + MAXITER
    return fits


@pytest.mark.parametrize("loop", ["fused", "resident"])
def test_keys_over_a_fit(loop, monkeypatch):
    """The starts take keys 0 .. nstarts - 1 (one launch from key0 = 0, or one objective-only step each); every later call
    starts where the one before it ended -- no gap, no reuse: a launch of n steps uses n keys -- and ends at nstarts + maxiter;
    one seed per fit, another one for the next fit, whose keys start at 0 again."""
    fits = _spied_fits(loop, monkeypatch)
    seeds = []
    for calls in fits:
        assert len({c[1] for c in calls}) == 1
        seeds.append(calls[0][1])
        assert 0 <= seeds[-1] < 2 ** 31 - 1
        nxt = 0
        for what, _, key, n in calls:
            assert key == nxt, (calls, what, key, nxt)
            nxt += n
        assert nxt == NSTARTS + MAXITER
        kinds = [c[0] for c in calls]
        if loop == "fused":
            assert calls[0][0] == "starts" and calls[0][3] == NSTARTS
            assert set(kinds[1:]) == {"run"} and len(kinds) > 2 and sum(c[3] for c in calls[1:]) == MAXITER
        else:
            assert kinds[:NSTARTS] == ["objective"] * NSTARTS and kinds[NSTARTS:] == ["step"] * MAXITER
    assert seeds[0] != seeds[1]
