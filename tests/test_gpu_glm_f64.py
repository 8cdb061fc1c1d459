"""`GeneralizedLinearModel(dtype="f64")`: the SVI step on the float64 feature matrix (rr_glm64.hip) against the reference's
golden step, the oracle on richer bases and ragged shapes, the likelihood terms per element at float64's bound, the row slabs
of the Ed product, the resident gather, the reference's fits at 1e-8 and the prediction's latent samples at 1e-12
(tests/glm_f64_cases.py: shapes, bound and tolerances).  The f32 step stands at 1e-3 .. 1e-4 on the same fixtures."""
import numpy as np
import pytest

import centres_cases as cc
import glm_f64_cases as gc
import lik_cases as lc
import revrand_oracle as orc
from conftest import normwise
from glm_fit_cases import IMPLEMENTED

pytestmark = pytest.mark.gpu


def _imports():
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd.btypes import Parameter, Positive
    from revrand_amd.glm import GeneralizedLinearModel
    return bs, lk, Parameter, Positive, GeneralizedLinearModel


def _lik(lk, name):
    return {"poisson_exp": lambda: lk.Poisson("exp"), "poisson_softplus": lambda: lk.Poisson("softplus"),
            "gaussian": lk.Gaussian, "bernoulli": lk.Bernoulli, "binomial": lk.Binomial}[name]()


def _flat(v):
    v = v if isinstance(v, (list, tuple)) else [v]
    return np.concatenate([np.ravel(np.asarray(u, dtype=float)) for u in v] + [np.empty(0)])


def _step(glm, m, C, regs, lp, hyp, X, y, *largs, **kw):
    glm._GeneralizedLinearModel__it = -1
    return glm._elbo(m.copy(), C.copy(), regs, lp, hyp, X, y, *largs, **kw)


def _check_step(got, want, label=""):
    """-ELBO and the gradient blocks of one step against the oracle's glm_elbo / the golden step, at the float64 tolerances."""
    nobj, (ndm, ndC, dL, dlp, dbp) = got
    wobj, (wdm, wdC, wdL, wdlp, wdbp) = want
    errs = {"obj": abs(nobj - wobj) / abs(wobj), "ndm": normwise(ndm, wdm), "ndC": normwise(ndC, wdC),
            "dL": normwise(_flat(dL), _flat(wdL))}
    if _flat(wdbp).size:
        errs["dbp"] = normwise(_flat(dbp), _flat(wdbp))
    if _flat(wdlp).size:
        errs["dlp"] = normwise(_flat(dlp), _flat(wdlp))
    print("float64 step %s: %s" % (label, {k: "%.2e" % v for k, v in errs.items()}))
    assert errs["obj"] < gc.TOL_OBJ, errs
    assert errs["dL"] < gc.TOL_DL, errs
    assert max(errs[k] for k in errs if k not in ("obj", "dL")) < gc.TOL_GRAD, errs
    return errs


# ---- 1: the reference's own step ---------------------------------------------------------------------------------------------
CASES = [("iso", n) for n in ("poisson_exp", "poisson_softplus", "gaussian", "bernoulli", "binomial")] \
    + [("ard", "poisson_exp"), ("ard", "gaussian")]


@pytest.mark.parametrize("tag,lik", CASES)
def test_minibatch_elbo_vs_reference(golden, tag, lik):
    """The seven cases of tests/golden/glm.npz (256 rows, d = 4, F = 64, K = 3, L = 8) through `_elbo`, as
    test_gpu_glm.py::test_minibatch_elbo_vs_reference runs them in float32 (2e-4 / 1e-3 / 2e-3 there)."""
    bs, lk, Parameter, Positive, GLM = _imports()
    g = golden("glm")
    X, K, L = g["X"], int(g["K"]), int(g["L"])
    d = X.shape[1]
    ls = g[tag + "_ls"]
    ls = float(ls) if np.ndim(ls) == 0 else ls
    lsp = Parameter(np.ones(d), Positive()) if tag == "ard" else Parameter(1., Positive())
    basis = bs.RandomRBF(nbases=32, Xdim=d, random_state=7, lenscale=lsp)
    assert np.array_equal(basis.W, g["W"])
    glm = GLM(likelihood=_lik(lk, lik), basis=basis, K=K, nsamples=L, random_state=int(g["seed"]), dtype="f64")
    glm.B_, glm.D_ = float(g["B"]), 64
    t = tag + "_" + lik
    lp = 0.7 if lik == "gaussian" else []
    largs = (g["nbin"],) if lik == "binomial" else ()
    try:
        got = _step(glm, g["m"], g["C"], float(g["reg"]), lp, ls, X, g[t + "_y"], *largs)
    finally:
        glm._release_features()
    assert np.shape(got[1][4]) == (() if tag == "iso" else (d,))
    want = (g[t + "_obj"], (g[t + "_ndm"], g[t + "_ndC"], g[t + "_dL"], g[t + "_dlp"] if lik == "gaussian" else [], g[t + "_dbp"]))
    _check_step(got, want, t)
    if lik != "gaussian":
        assert got[1][3] == []


# ---- 2: ragged concatenations against the oracle ---------------------------------------------------------------------------
def _pad_slabs(Phi, blocks, grads):
    """Every child's gradient slabs, zero padded to the concatenation's width, in concatenation order."""
    ends = np.cumsum([0] + [b.shape[1] for b in blocks])
    out = []
    for i, g in enumerate(grads):
        for s in g:
            full = np.zeros_like(Phi)
            full[:, ends[i]:ends[i + 1]] = s
            out.append(full)
    return out


def _slices3(g):
    return [g] if g.ndim == 2 else [g[:, :, i] for i in range(g.shape[2])]


def _concat(every):
    """The basis of test_gpu_glm.py::test_minibatch_elbo_concat_and_generic_children_vs_oracle (RandomMatern32 ARD + LinearBasis +
    FastFoodGM through the generic child + RandomRBF on a column subset) -- `every`: with a RadialBasis and a PolynomialBasis
    child (device children under resident_bases="all").  Returns (basis, hypers, regs, Phi, slabs) with Phi and the gradient
    slabs restated in NumPy float64 (the oracle's and centres_cases' formulas)."""
    bs, lk, Parameter, Positive, GLM = _imports()
    d = gc.CONCAT["d"]
    rs = np.random.RandomState(3)
    X = rs.randn(gc.CONCAT["M"], d)
    b0 = bs.RandomMatern32(nbases=40, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
    b1 = bs.LinearBasis(onescol=True)
    b2 = bs.FastFoodGM(nbases=8, Xdim=2, random_state=2, apply_ind=[1, 3], dtype="f64")   # its own transform / grad: float64
    b3 = bs.RandomRBF(nbases=30, Xdim=2, random_state=4, apply_ind=[0, 2])
    ls0, mu, lsg, ls3 = np.linspace(0.8, 1.3, d), np.array([0.3, -0.2]), np.array([1.1, 0.9]), 0.7
    X2, X3 = X[:, [1, 3]], X[:, [0, 2]]
    blocks = [orc.rff_transform(X, b0.W, ls0), orc.linear_transform(X, True),
              orc.fastfood_gm_transform(X2, b2.B, b2.G, b2.PI, b2.S, mu, lsg), orc.rff_transform(X3, b3.W, ls3)]
    dM, dLs = orc.fastfood_gm_grad(X2, b2.B, b2.G, b2.PI, b2.S, mu, lsg)
    grads = [_slices3(orc.rff_grad(X, b0.W, ls0)), [], _slices3(dM) + _slices3(dLs), _slices3(orc.rff_grad(X3, b3.W, ls3))]
    bases, hyp, regs = [b0, b1, b2, b3], [ls0, mu, lsg, ls3], [1.2, 0.8, 1.5, 0.6]
    if every:
        Cc = rs.randn(9, 3)
        lsr = np.array([0.9, 1.2, 1.05])
        b4 = bs.RadialBasis(Cc, lenscale=Parameter(np.ones(3), Positive()), apply_ind=[0, 2, 4])
        b5 = bs.PolynomialBasis(order=3, include_bias=False, apply_ind=[1, 2])
        X4 = X[:, [0, 2, 4]]
        blocks += [cc.radial_transform(X4, Cc, lsr), cc.poly_transform(X[:, [1, 2]], 3, False)]
        grads += [_slices3(cc.radial_grad(X4, Cc, lsr)), []]
        bases, hyp, regs = bases + [b4, b5], hyp + [lsr], regs + [0.9, 1.1]
    cat = bases[0]
    for b in bases[1:]:
        cat = cat + b
    Phi = np.hstack(blocks)
    return X, cat, hyp, regs, Phi, _pad_slabs(Phi, blocks, grads)


@pytest.mark.parametrize("every", [False, True], ids=["fourier", "all"])
def test_ragged_concatenation_vs_oracle(every):
    """M = 333, d = 5, K = 4, L = 7: nothing a multiple of anything; device children (random Fourier, linear -- and centre /
    polynomial under resident_bases="all") next to a generic child whose gradient is formed on the host from the downloaded
    EdPhi block."""
    bs, lk, Parameter, Positive, GLM = _imports()
    K, L = gc.CONCAT["K"], gc.CONCAT["L"]
    X, cat, hyp, regs, Phi, slabs = _concat(every)
    rs = np.random.RandomState(5)
    y = rs.poisson(np.exp(0.5 * np.sin(X[:, 0]))).astype(float)
    D = Phi.shape[1]
    assert D == int(cat.get_dim(X))
    m = 0.2 * rs.randn(D, K)
    C = rs.gamma(2., 0.5, size=(D, K))
    Ld, slices = cat.regularizer_diagonal(X, *regs)
    e = np.random.RandomState(9).randn(K * L, D).reshape(K, L, D)
    want = orc.glm_elbo(m, C, Ld, slices, "poisson_exp", [], (), Phi, slabs, y, e, 6.0)
    glm = GLM(likelihood=lk.Poisson(), basis=cat, K=K, nsamples=L, random_state=9, dtype="f64",
              resident_bases="all" if every else "fourier")
    glm.B_, glm.D_ = 6.0, D
    try:
        got = _step(glm, m, C, regs, [], hyp, X, y)
        kinds = [type(c).__name__ for c, _, _ in glm._features().children]
    finally:
        glm._release_features()
    assert kinds == ["_ResidentRFF", "_ResidentLinear", "_ResidentGeneric", "_ResidentRFF"] + (["_ResidentCentres", "_ResidentPoly"] if every else [])
    dbp = got[1][4]
    assert isinstance(dbp, list) and len(dbp) == (5 if every else 4)
    _check_step(got, want, "concat/" + ("all" if every else "fourier"))


# ---- 3 / 5: every tile edge at once; the row slabs; the Gaussian ------------------------------------------------------------
def _edges(lik):
    bs, lk, Parameter, Positive, GLM = _imports()
    M, n, K, L, d = (gc.EDGES[k] for k in ("M", "n", "K", "L", "d"))
    rs = np.random.RandomState(11)
    X = rs.randn(M, d)
    basis = bs.RandomRBF(nbases=n, Xdim=d, random_state=6, lenscale=Parameter(np.ones(d), Positive()))
    ls = np.linspace(0.9, 1.4, d)
    Phi = orc.rff_transform(X, basis.W, ls)
    slabs = _slices3(orc.rff_grad(X, basis.W, ls))
    D = 2 * n
    m = 0.1 * rs.randn(D, K)
    C = rs.gamma(2., 0.05, size=(D, K))
    if lik == "gaussian":
        y = np.sin(X[:, 0]) + 0.1 * rs.randn(M)
    else:
        y = rs.poisson(np.exp(0.5 * np.sin(X[:, 0]))).astype(float)
    return X, y, basis, ls, Phi, slabs, m, C


def _edge_model(lik, basis, seed=13):
    bs, lk, Parameter, Positive, GLM = _imports()
    glm = GLM(likelihood=_lik(lk, lik), basis=basis, K=gc.EDGES["K"], nsamples=gc.EDGES["L"], random_state=seed, dtype="f64")
    glm.B_, glm.D_ = 4.0, 2 * gc.EDGES["n"]
    return glm


def _bytes(res, basis_grads=True):
    """The step's results as bytes.  basis_grads=False: without dbp -- the one output that is not the step's own: the random
    Fourier children's contraction (rr_glm_grad_t64_kernel) adds its row blocks' partials with float64 atomics unless the context
    is deterministic, exactly like the second pass' rr_grad_t64_kernel, so its last bits move from run to run in the default mode."""
    nobj, (ndm, ndC, dL, dlp, dbp) = res
    parts = (nobj, ndm, ndC, _flat(dL), _flat(dlp)) + ((_flat(dbp),) if basis_grads else ())
    return b"".join(np.ascontiguousarray(np.asarray(v, dtype=float)).tobytes() for v in parts)


class _Deterministic(object):
    """rr_set_deterministic for a block (restored on the way out)."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from revrand_amd import _hip
        self.dev = _hip.get_device()
        self.prev = self.dev.set_deterministic(self.on)

    def __exit__(self, *exc):
        self.dev.set_deterministic(self.prev)


def test_every_tile_edge_and_the_row_slabs(monkeypatch):
    """300 rows, F = 200, K L = 150: two or three ragged 128-tiles in each dimension of each product.  RR_GLM64_KSLABS = 1 and = 3
    (slabs of 128 padded rows: 128 + 128 + 44 data rows): each against the oracle, each twice with identical bytes, the two
    within 1e-12 of each other.  Identical bytes: everything the step itself returns (-ELBO, dm, dC, dL) in either determinism
    mode -- it has no floating-point atomics -- and the basis gradient too once the context is deterministic (`_bytes`)."""
    K, L = gc.EDGES["K"], gc.EDGES["L"]
    X, y, basis, ls, Phi, slabs, m, C = _edges("poisson_exp")
    D = Phi.shape[1]
    e = np.random.RandomState(13).randn(K * L, D).reshape(K, L, D)
    want = orc.glm_elbo(m, C, np.full(D, 1.3), [slice(0, D)], "poisson_exp", [], (), Phi, slabs, y, e, 4.0)
    res = {}
    for det in (False, True):
        for nsl in ("1", "3"):
            monkeypatch.setenv("RR_GLM64_KSLABS", nsl)
            runs = []
            with _Deterministic(det):
                for _ in range(2):
                    glm = _edge_model("poisson_exp", basis)
                    try:
                        runs.append(_step(glm, m, C, 1.3, [], ls, X, y))
                    finally:
                        glm._release_features()
            _check_step(runs[0], want, "edges, %s slab(s)%s" % (nsl, ", deterministic" if det else ""))
            assert _bytes(runs[0], basis_grads=det) == _bytes(runs[1], basis_grads=det), "two runs with %s slab(s) differ" % nsl
            if det:   # the step's own results do not depend on the mode
                assert _bytes(runs[0], False) == _bytes(res[nsl], False)
            res[nsl] = runs[0]
    a, b = res["1"], res["3"]
    diff = {"ndm": normwise(a[1][0], b[1][0]), "ndC": normwise(a[1][1], b[1][1]), "dbp": normwise(_flat(a[1][4]), _flat(b[1][4])),
            "obj": abs(a[0] - b[0]) / abs(a[0])}
    print("one slab against three: %s" % {k: "%.2e" % v for k, v in diff.items()})
    assert max(diff.values()) < gc.TOL_SLABS, diff


def test_gaussian_sums_and_the_objective_only_route():
    """The shape of the tile-edge test under the Gaussian: aux = sum (y - f)^2 and llsum = -aux / (2 var) per component against
    NumPy, dlp against the oracle's lik_dp (through glm_elbo), and the objective-only route's sums and -ELBO equal to the full
    step's bit for bit."""
    K, L = gc.EDGES["K"], gc.EDGES["L"]
    var = 0.7
    X, y, basis, ls, Phi, slabs, m, C = _edges("gaussian")
    D = Phi.shape[1]
    E = np.random.RandomState(13).randn(K * L, D)
    want = orc.glm_elbo(m, C, np.full(D, 1.3), [slice(0, D)], "gaussian", [var], (), Phi, slabs, y, E.reshape(K, L, D), 4.0)
    glm = _edge_model("gaussian", basis)
    try:
        full = _step(glm, m, C, 1.3, var, ls, X, y)
        glm.random_ = np.random.RandomState(13)
        only = _step(glm, m, C, 1.3, var, ls, X, y, objective_only=True)
        f = glm._features()
        f.assemble(X, [ls])
        Edm, EdC, ll, aux = f.glm_step_draws(y, None, lc.LIK_ID["gaussian"], var, m, C, K, L, E)
        f.assemble(X, [ls])
        none_m, none_C, ll_o, aux_o = f.glm_step_draws(y, None, lc.LIK_ID["gaussian"], var, m, C, K, L, E, objective_only=True)
    finally:
        glm._release_features()
    _check_step(full, want, "edges, gaussian")
    assert only == full[0]
    assert none_m is None and none_C is None
    assert ll_o.tobytes() == ll.tobytes() and aux_o.tobytes() == aux.tobytes()
    ws = (m.T[:, None, :] + np.sqrt(C.T)[:, None, :] * E.reshape(K, L, D))          # (K, L, D)
    sq = ((y[None, None, :] - ws @ Phi.T) ** 2).sum(axis=(1, 2))
    assert normwise(aux, sq) < 1e-12 and normwise(ll, -0.5 * sq / var) < 1e-12
    dp = np.array([orc.lik_dp("gaussian", y, ws[k] @ Phi.T, var)[0].sum() for k in range(K)])
    assert normwise(0.5 * (aux / var ** 2 - y.size * L / var), dp) < 1e-12


# ---- 4: the likelihood terms per element -------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", lc.LIKS)
def test_every_grid_point_per_element(lik):
    """One row, one feature, X = [[1]], L = 1, the weight samples the grid (lik_cases' 64 values and +-36.7, +-36.8: K = 68; the
    samples are not pre-scaled, so f is the sample itself for any K): Edws[:, 0] is df and llsum[k] is ll of element k -- every one
    within (16 + 4 |f|) 2^-53 S + 1e-300, for every target and every binomial n, float64 targets; llsum once more on the
    objective-only route (m the grid, C = 1e-300, zero draws)."""
    from revrand_amd import basis_functions as bs
    grid = gc.grid(lik)
    lid, K = lc.LIK_ID[lik], grid.size
    X = np.ones((1, 1))
    WS = grid[:, None].copy()
    fails, top = [], {"df": 0.0, "ll": 0.0, "ll objective": 0.0}

    def check(what, got, want, S, y, n):
        i, r = lc.worst(got, want, gc.bound(grid, S))
        top[what] = max(top[what], r)
        if not r <= 1:
            fails.append("%s %s: y=%g n=%g f=%r got=%r want=%r ratio to the bound=%.4g" % (lik, what, y, n, float(grid[i]),
                                                                                         float(got[i]), float(want[i]), r))
    f = bs.MinibatchFeatures64(bs.LinearBasis(onescol=False))
    try:
        for y, n in lc.targets(lik):
            ya, na = np.array([y]), np.array([n]) if lik == "binomial" else None
            want_df, want_ll = lc.ref_df(lik, y, grid, n), lc.ref_ll(lik, y, grid, n)
            S_df, S_ll = lc.s_df(lik, y, grid, n), lc.s_ll(lik, y, grid, n)
            f.assemble(X, [])
            Edws, ll, _ = f.glm_step(ya, na, lid, 0.0, WS, K, 1)
            assert Edws.shape == (K, 1) and ll.shape == (K,)
            check("df", Edws[:, 0], want_df, S_df, y, n)
            check("ll", ll, want_ll, S_ll, y, n)
            f.assemble(X, [])
            _, _, ll, _ = f.glm_step_draws(ya, na, lid, 0.0, WS.T.copy(), np.full((1, K), 1e-300), K, 1, np.zeros((K, 1)),
                                           objective_only=True)
            check("ll objective", ll, want_ll, S_ll, y, n)
    finally:
        f.release()
    for what in sorted(top):
        print("worst ratio to the float64 bound: %-12s %-17s %.3g" % (what, lik, top[what]))
    assert not fails, "%d (target, output) pairs outside the bound; the worst element of each:\n%s" % (len(fails), "\n".join(fails))


# ---- 6: rows gathered on the device by index ------------------------------------------------------------------------------------
def test_resident_gather_equals_host_rows_bit_for_bit():
    """The shape of the ragged concatenation with children that can all gather float64 rows (random Fourier, linear, radial,
    polynomial; resident_bases="all"): `_elbo` on rows gathered on the device by index against `_elbo` on the same rows assembled
    from the host.  In the default mode everything the step returns, and with a deterministic context the basis gradient as well
    (`_bytes`: the random Fourier contraction's atomics)."""
    bs, lk, Parameter, Positive, GLM = _imports()
    d, K, L, M = gc.CONCAT["d"], gc.CONCAT["K"], gc.CONCAT["L"], gc.CONCAT["M"]
    rs = np.random.RandomState(21)
    N = 500
    X = rs.randn(N, d)
    y = rs.poisson(np.exp(0.5 * np.sin(X[:, 0]))).astype(float)
    Cc = rs.randn(9, 3)
    cat = bs.RandomMatern32(nbases=40, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive())) \
        + bs.LinearBasis(onescol=True) + bs.RandomRBF(nbases=30, Xdim=2, random_state=4, apply_ind=[0, 2]) \
        + bs.RadialBasis(Cc, lenscale=Parameter(np.ones(3), Positive()), apply_ind=[0, 2, 4]) \
        + bs.PolynomialBasis(order=3, include_bias=False, apply_ind=[1, 2])
    hyp, regs = [np.linspace(0.8, 1.3, d), 0.7, np.array([0.9, 1.2, 1.05])], [1.2, 0.8, 0.6, 0.9, 1.1]
    D = int(cat.get_dim(X))
    m = 0.2 * rs.randn(D, K)
    C = rs.gamma(2., 0.5, size=(D, K))
    idx = rs.permutation(N)[:M]

    def model():
        glm = GLM(likelihood=lk.Poisson(), basis=cat, K=K, nsamples=L, random_state=9, dtype="f64", resident_bases="all")
        glm.B_, glm.D_ = 6.0, D
        return glm
    for det in (False, True):
        with _Deterministic(det):
            host = model()
            try:
                a = _step(host, m, C, regs, [], hyp, X[idx], y[idx])
            finally:
                host._release_features()
            res = model()
            try:
                assert res._features().make_resident(X, "all") is True
                res._resident_fit = True
                b = _step(res, m, C, regs, [], hyp, X[idx], y[idx], idx)
                kinds = [type(c).__name__ for c, _, _ in res._features().children]
            finally:
                res._resident_fit = False
                res._release_features()
        assert kinds == ["_ResidentRFF", "_ResidentLinear", "_ResidentRFF", "_ResidentCentres", "_ResidentPoly"]
        assert _bytes(a, basis_grads=det) == _bytes(b, basis_grads=det)
        assert normwise(_flat(a[1][4]), _flat(b[1][4])) < 1e-13


# ---- 7: the reference's fits -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", IMPLEMENTED, ids=[c[0] for c in IMPLEMENTED])
def test_fit_equals_the_references_fit(golden, case, monkeypatch):
    """Every implemented case of tests/golden/glm_fit.npz with dtype="f64": the fitted blocks within 1e-8 normwise (the f32 loops:
    1e-4), the random stream ending in the reference's state, the host loop around `_elbo` with one float64 library call per
    step and per random start -- and neither device loop."""
    from revrand_amd import _hip
    from test_gpu_glm_fit import _model
    g = golden("glm_fit")
    tag, lik = case[0], case[1]
    glm, largs = _model(g, case)
    glm.set_params(dtype="f64")
    calls = {"resident": 0, "fused": 0, "f64 steps": 0, "f64 objectives": 0}
    real, real_run, real64 = _hip.ResidentSgd.step, _hip.FusedSvi.run, _hip.FeatureMatrix64.glm_step_draws

    def spy(self, *a, **k):
        calls["resident"] += 1
        return real(self, *a, **k)

    def spy_run(self, n, *a, **k):
        calls["fused"] += n
        return real_run(self, n, *a, **k)

    def spy64(self, *a, **k):
        calls["f64 objectives" if k.get("objective_only") or (len(a) > 9 and a[9]) else "f64 steps"] += 1
        return real64(self, *a, **k)
    monkeypatch.setattr(_hip.ResidentSgd, "step", spy)
    monkeypatch.setattr(_hip.FusedSvi, "run", spy_run)
    monkeypatch.setattr(_hip.FeatureMatrix64, "glm_step_draws", spy64)
    np.random.seed(int(g["global_seed"]))
    glm.fit(g["X"], g["y_" + ("poisson_exp" if lik == "poisson_softplus" else lik)], likelihood_args=largs)
    assert calls == {"resident": 0, "fused": 0, "f64 steps": int(g["maxiter"]), "f64 objectives": case[4]}
    errs = {"m": normwise(glm.weights_, g[tag + "_m"]), "C": normwise(glm.covariance_, g[tag + "_C"]),
            "reg": normwise(_flat(glm.regularizer_), g[tag + "_reg"]), "ls": normwise(_flat(glm.basis_hypers_), g[tag + "_ls"])}
    if lik == "gaussian":
        errs["lik"] = normwise(_flat(glm.like_hypers_), g[tag + "_lik"])
    print("float64 fit %-34s %s" % (tag, {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) < gc.TOL_FIT, errs
    assert glm.random_.randn() == float(g[tag + "_end"])


# ---- 8: prediction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lik", ["gaussian", "poisson_exp", "binomial"])
def test_latent_samples_vs_reference(golden, lik):
    """`_sample_matrix` (randint then randn from `random_`, the product on the float64 matrix) against the reference's recorded
    latent samples at 1e-12 normwise -- the oracle's own figure; the f32 projection stands at 1e-5."""
    bs, lk, Parameter, Positive, GLM = _imports()
    g = golden("glm_predict")
    X, K, S = g["X"], int(g["K"]), int(g["S"])
    basis = bs.LinearBasis(onescol=True) + bs.RandomRBF(nbases=g["W"].shape[1], Xdim=X.shape[1], random_state=8)
    assert np.array_equal(basis.bases[1].W, g["W"])
    glm = GLM(_lik(lk, lik), basis, K=K, random_state=0, dtype="f64")
    glm.weights_, glm.covariance_, glm.regularizer_ = g["m"], g["C"], [1.0, 1.0]
    glm.like_hypers_ = 0.3 if lik == "gaussian" else []
    glm.basis_hypers_ = float(g["ls"])
    glm.random_ = np.random.RandomState(77)
    try:
        fs = glm._sample_matrix(X, S)
    finally:
        glm._drop_serving()
    err = normwise(fs.T, g[lik + "_fs"])
    print("float64 latent samples %-12s %.2e" % (lik, err))
    assert err < gc.TOL_PROJECT


@pytest.mark.parametrize("S", [1, 130])
def test_project_one_and_many_samples(S):
    """rr_featmat64_project with one sample and with 130 (two column tiles, the second ragged) on 333 ragged rows."""
    bs, lk, Parameter, Positive, GLM = _imports()
    X, cat, hyp, regs, Phi, _ = _concat(False)
    W = np.random.RandomState(S).randn(Phi.shape[1], S)
    f = bs.MinibatchFeatures64(cat)
    try:
        out = f.project(X, hyp, W)
    finally:
        f.release()
    assert out.shape == (X.shape[0], S)
    assert normwise(out, Phi @ W) < gc.TOL_PROJECT


# ---- 9: refusals -----------------------------------------------------------------------------------------------------------------
def test_refusals_are_error_codes_before_any_launch():
    from revrand_amd import _hip
    import revrand_amd.basis_functions as bs
    rs = np.random.RandomState(2)
    rows, d, n, K, L = 40, 3, 8, 2, 3
    X = rs.randn(rows, d)
    basis = bs.RandomRBF(nbases=n, Xdim=d, random_state=1)
    h = basis._handle()
    dev = _hip.get_device()
    F = 2 * n + d + 1
    fm = _hip.FeatureMatrix64(rows, F)
    dXr = h.upload(np.ascontiguousarray(X, dtype=np.float64))
    dXl = dev.upload_matrix(X)
    dy = dev.upload_vector(rs.poisson(1.0, rows).astype(float), np.float64)
    dn = dev.upload_vector(np.full(rows, 5.0), np.float64)
    dT = dev.zeros(d * n * 8)
    WS = 0.1 * rs.randn(K * L, F)
    m, C, E = 0.1 * rs.randn(F, K), np.full((F, K), 0.5), rs.randn(K * L, F)

    def refused(fn, *a, **k):
        with pytest.raises(_hip.HipError) as ei:
            fn(*a, **k)
        assert ei.value.code != 0 and str(ei.value)
        return str(ei.value)
    try:
        # an incomplete matrix: only the random Fourier block was put
        fm.begin(rows)
        fm.put_rff(h, dXr, 1.0, 0)
        assert "columns were written" in refused(fm.glm_step, dy, None, lc.LIK_ID["poisson_exp"], 0.0, WS, K, L)
        assert "columns were written" in refused(fm.glm_step_draws, dy, None, lc.LIK_ID["poisson_exp"], 0.0, m, C, K, L, E)
        assert "columns were written" in refused(fm.project, rows, WS.T.copy())
        fm.put_linear(dXl, True, 2 * n)
        # a binomial without its n, a variance that is not positive, K L >= 2^24, the contractions before any step
        assert "binomial" in refused(fm.glm_step, dy, None, lc.LIK_ID["binomial"], 0.0, WS, K, L)
        assert "variance" in refused(fm.glm_step, dy, None, lc.LIK_ID["gaussian"], 0.0, WS, K, L)
        assert "rr_featmat64_glm_step first" in refused(fm.glm_rff, h, dXr, 0, dT)
        assert "rr_featmat64_glm_step first" in refused(fm.glm_edphi, rows, 0, F)
        # a step, then the second pass: EdPhi is gone -- and after the next step the second pass' rows are
        fm.glm_step(dy, dn, lc.LIK_ID["binomial"], 0.0, WS, K, L)
        fm.glm_rff(h, dXr, 0, dT)
        assert fm.glm_edphi(rows, 0, F).shape == (rows, F)
        fm.pass2_begin(np.zeros(F), np.eye(F))
        assert "rr_featmat64_glm_step first" in refused(fm.glm_rff, h, dXr, 0, dT)
        assert "rr_featmat64_glm_step first" in refused(fm.glm_edphi, rows, 0, F)
        fm.pass2_rows(dy)
        fm.pass2_rff(h, dXr, 0, dT)
        assert "rr_featmat64_glm_step first" in refused(fm.glm_rff, h, dXr, 0, dT)
        fm.glm_step_draws(dy, None, lc.LIK_ID["poisson_exp"], 0.0, m, C, K, L, E)
        assert "pass2_rows first" in refused(fm.pass2_rff, h, dXr, 0, dT)
        fm.glm_rff(h, dXr, 0, dT)
        # begin: EdPhi belonged to the rows it was formed from
        fm.begin(rows)
        fm.put_rff(h, dXr, 1.0, 0)
        fm.put_linear(dXl, True, 2 * n)
        assert "rr_featmat64_glm_step first" in refused(fm.glm_rff, h, dXr, 0, dT)
        assert "rr_featmat64_glm_step first" in refused(fm.glm_edphi, rows, 0, F)
        # an objective-only step stores no EdPhi
        fm.glm_step_draws(dy, None, lc.LIK_ID["poisson_exp"], 0.0, m, C, K, L, E, objective_only=True)
        assert "rr_featmat64_glm_step first" in refused(fm.glm_rff, h, dXr, 0, dT)
        dev.sync()
    finally:
        for b in (dXr, dXl, dy, dn, dT):
            b.free()
