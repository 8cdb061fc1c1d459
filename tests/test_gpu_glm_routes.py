"""Every kernel route of the GLM step's three products and of `project` against float64.

fm_gemm (rr_elbo.hip:1756-1813) picks a kernel from the shape and the CU count, glm_pipeline (:2782-2886) may replace the
first product by the likelihood-epilogue kernel and the third by the fused contraction, and rr_featmat_project
(:3080-3130) takes a dot-product kernel for one vector.  `step_routes` / `project_route` restate those rules; the cases
below are chosen so that, on the MI355X's 256 CUs, they hit every route, split K with a shorter last split, and (where K
is the row count) keep data in the last 32-row k-block.

On integer data (features in {-1, 0, 1}, small integer targets, a Gaussian likelihood with a power-of-two variance, K L a
power of two) every f32 route returns the exact result whatever its summation order or atomics, as long as the sum of
|a_i| |b_i| of every output stays below 2^24 -- checked on the host -- so those outputs are compared BIT FOR BIT: a
dropped or doubled k-block cannot hide inside a tolerance.  Config 5's routes with realistic features (RandomRBF, ARD,
Poisson) are held to the oracle with the suite's usual tolerances."""
import os

import numpy as np
import pytest

import revrand_oracle as orc
from conftest import normwise

pytestmark = pytest.mark.gpu

EXACT = 1 << 24
KERNEL = {"small": "rr_gemm_tn_small_f32_kernel", "mid_split": "rr_gemm_tn_mid_f32_kernel", "mid": "rr_gemm_tn_mid_f32_kernel",
          "tile": "rr_gemm_tn_f32_kernel", "tile_split": "rr_gemm_tn_f32_kernel", "lik": "rr_gemm_lik_f32_kernel",
          "gradt": "rr_gemm_gradt_f32_kernel", "rowvec": "rr_rowvec_kernel"}
GEMM_KERNELS = sorted(set(KERNEL.values()))


# ---- the route table ----------------------------------------------------------------------------------------------------
def _r256(n):
    return (n + 255) // 256 * 256


def _is_small(K, M, N):  # fm_gemm_is_small, rr_elbo.hip:1763
    return K * M * N <= (1 << 27) and M // 32 < 65536


def _is_mid(K, M, N, cu, det):  # fm_gemm_is_mid, rr_elbo.hip:1756
    return not det and (M // 256) * (N // 256) * 4 <= cu and K <= 4096 and K % 32 == 0 and M % 128 == 0 and N % 128 == 0


def gemm_route(K, M, N, cu, det):
    """fm_gemm (rr_elbo.hip:1768-1813) with the default RR_GEMM_MID_ROUNDS = 2 and RR_GEMM_SPLIT_ROUNDS = 1: (route, K-splits,
    k-blocks per split, k-blocks of the last split).  With K >= 256 (every product here) the mid kernel always splits."""
    nkb = K // 32
    if _is_small(K, M, N):
        return ("small", 1, nkb, nkb)
    if _is_mid(K, M, N, cu, det):
        tiles = (M // 128) * (N // 128)
        want = min(-(-2 * cu // tiles), nkb // 4)  # :1783-1784
        if want > 1:
            kbps = -(-nkb // want)
            splits = -(-nkb // kbps)
            return ("mid_split", splits, kbps, nkb - (splits - 1) * kbps)
        return ("mid", 1, nkb, nkb)
    tiles = (M // 256) * (N // 256)
    if tiles < 2 * cu and nkb >= 16:  # :1799-1807
        want = min(-(-cu // tiles), nkb // 8)
        kbps = -(-nkb // want)
        splits = -(-nkb // kbps)
        return ("tile_split", splits, kbps, nkb - (splits - 1) * kbps)
    return ("tile", 1, nkb, nkb)


def step_routes(rows, F, KL, cu, det=False, fuse_lik="auto", lone_rff=False, klp=None):
    """The step's products (glm_pipeline, rr_elbo.hip:2782-2886) for the default Gram engine: fs (K = Fp, M = rows256, N = klp),
    Ed (K = rows256, M = klp, N = Fp), EdPhi (K = klp, M = rows256, N = Fp).  klp: the scratch's sample width when a
    feature matrix saw a wider step or projection before (fm_glm_scratch only grows)."""
    rows256, Fp = _r256(rows), _r256(F)
    klp = klp or _r256(KL)
    tiles1 = (rows256 // 256) * (klp // 256)
    small = fuse_lik != "force" and _is_small(Fp, rows256, klp)  # :2820
    lik_auto = tiles1 >= 2 * cu or Fp // 32 < 16  # :2818
    take_lik = not det and fuse_lik != "0" and (fuse_lik == "force" or lik_auto) and not small  # :2821
    fs = ("lik", 1, Fp // 32, Fp // 32) if take_lik else gemm_route(Fp, rows256, klp, cu, det)
    ed = gemm_route(rows256, klp, Fp, cu, det)
    # :2797-2800 (a lone random Fourier child of Xdim <= 128 whose [cos | sin] block is the whole, 256-aligned matrix)
    gradt = lone_rff and not det and not _is_mid(klp, rows256, Fp, cu, det) and F == Fp and (F // 2) % 256 == 0
    edphi = ("gradt", 1, klp // 32, klp // 32) if gradt else gemm_route(klp, rows256, Fp, cu, det)
    return {"fs": fs, "Ed": ed, "EdPhi": edphi}


def project_route(rows, F, S, cu, det=False, ldw=None):
    """rr_featmat_project (rr_elbo.hip:3080-3130): one vector on rr_rowvec_kernel, else fm_gemm with K = Fp, M = rows256,
    N = S rounded up to 256 (or the scratch's wider sample width)."""
    if S == 1:
        return ("rowvec", 1, 0, 0)
    return gemm_route(_r256(F), _r256(rows), ldw or _r256(S), cu, det)


# ---- the cases ----------------------------------------------------------------------------------------------------------
# (rows, F, K, L): K L a power of two; rows and F off the 256 grid
STEP_CASES = [(300, 300, 32, 16),      # every product on the small kernel (and the epilogue kernel when forced)
              (200, 4300, 32, 32),     # Ed: one 256-row k-range, tiles only (no split); fs: tile split; EdPhi: mid split
              (2000, 700, 32, 32),     # all three on the mid kernel, Ed and EdPhi with a shorter last split
              (4350, 1000, 32, 16),    # fs: mid split; Ed: tile split over a k-range whose last block holds rows
              (16884, 500, 32, 16),    # Ed: 59 splits of 9 k-blocks, the last of 6, holding rows 16864-16883
              (65536, 500, 32, 16)]    # config 5's row count: the epilogue kernel, Ed tile split, EdPhi single pass
MODES = ["auto", "force", "0", "det"]  # RR_GLM_FUSE_LIK unset / force / 0; deterministic mode
# (rows, F, S)
PROJECT_CASES = [(700, 300, 1), (700, 300, 33), (5000, 500, 300), (2000, 5370, 300), (16884, 2040, 300),
                 (65536, 300, 700)]
# config 5's routes with realistic features: rows, F = 2048 (1024 random Fourier bases), K L = 500, d <= 8
RFF_ROWS = [4352, 16384 + 300, 65536]
RFF_K, RFF_L, RFF_N, RFF_D = 10, 50, 1024, 6
SEQUENCE = [  # (rows, K, L, what) on ONE MinibatchFeatures of F = 500
    (300, 32, 16, "step"), (300, 32, 16, "step"), (5000, 32, 16, "step"), ("project", 300, 0, "project"),
    (300, 32, 32, "step"), (4350, 32, 32, "objective"), (4350, 32, 32, "step"), (65536, 16, 16, "step"),
    (1, 16, 16, "step"), (257, 16, 16, "step"), (4350, 32, 16, "step")]
SEQ_F = 500


def route_cases(cu):
    """(label, product, route) of every case the tests below run, at this CU count."""
    out = []
    for rows, F, K, L in STEP_CASES:
        for mode in MODES:
            r = step_routes(rows, F, K * L, cu, det=mode == "det", fuse_lik=mode if mode in ("force", "0") else "auto")
            out += [("step%s/%s" % ((rows, F, K, L), mode), p, v) for p, v in r.items()]
    for rows, F, S in PROJECT_CASES:
        out.append(("project%s" % ((rows, F, S),), "project", project_route(rows, F, S, cu)))
    for rows in RFF_ROWS:
        r = step_routes(rows, 2 * RFF_N, RFF_K * RFF_L, cu, lone_rff=True)
        out += [("rff%d" % rows, p, v) for p, v in r.items()]
    return out


# ---- integer data and its exact results ---------------------------------------------------------------------------------
def _tern(rs, shape, p):
    """Entries in {-1, 0, 1}, nonzero with probability p."""
    return (rs.choice([-1.0, 0.0, 1.0], size=shape, p=[p / 2, 1 - p, p / 2]))


def _exact_data(seed, rows, F, KL):
    rs = np.random.RandomState(seed)
    X = _tern(rs, (rows, F), 0.15)
    WS = _tern(rs, (KL, F), min(0.5, 6.0 / F))
    y = rs.randint(-2, 3, size=rows).astype(float)
    return X, y, WS


VAR = 0.5  # a power of two: dfs = (y - f) / VAR and llsum = -aux / (2 VAR) are exact


def _step_reference(X, y, WS, K, L):
    """Edws, llsum, aux, EdPhi of rr_featmat_glm_step in float64, after checking that every output is a sum of integers
    (scaled by a power of two) whose absolute terms stay below 2^24."""
    fs = X @ WS.T
    e = y[:, None] - fs
    aX, ae = np.abs(X), np.abs(e)
    assert (aX @ np.abs(WS).T).max() < EXACT
    assert (ae.T @ aX).max() < EXACT and (ae @ np.abs(WS)).max() < EXACT
    aux = (e * e).reshape(len(y), K, L).sum(axis=(0, 2))
    assert aux.max() < EXACT
    dfs = e / VAR
    return dfs.T @ X, -0.5 * aux / VAR, aux, dfs @ WS / (K * L)


def _assert_bitwise(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got != want
    assert not bad.any(), "%s: %d of %d differ, max |diff| %g" % (what, int(bad.sum()), bad.size, np.abs(got - want).max())


def _device():
    from revrand_amd import _hip
    return _hip.get_device()


class _Mode(object):
    """RR_GLM_FUSE_LIK (read per call) or deterministic mode for the duration of a block."""

    def __init__(self, mode):
        self.mode = mode

    def __enter__(self):
        self.env = os.environ.get("RR_GLM_FUSE_LIK")
        if self.mode in ("force", "0"):
            os.environ["RR_GLM_FUSE_LIK"] = self.mode
        else:
            os.environ.pop("RR_GLM_FUSE_LIK", None)
        self.det = _device().set_deterministic(self.mode == "det")
        return self

    def __exit__(self, *exc):
        _device().set_deterministic(self.det)
        if self.env is None:
            os.environ.pop("RR_GLM_FUSE_LIK", None)
        else:
            os.environ["RR_GLM_FUSE_LIK"] = self.env


def _linear_features():
    import revrand_amd.basis_functions as bs
    return bs.MinibatchFeatures(bs.LinearBasis(onescol=False))


def run_exact_step(f, X, y, WS, K, L, objective_only=False):
    """One step of integer data on MinibatchFeatures f: (Edws, llsum, aux, EdPhi), or (llsum, aux) for an objective-only one
    (glm_step_draws with m = 0, C = 1 and the weight samples as the draws: the same w / (K L))."""
    from revrand_amd import likelihoods as lk
    f.assemble(X, [])
    if objective_only:
        F = X.shape[1]
        _, _, ll, aux = f.glm_step_draws(y, None, lk.RR_LIK_GAUSSIAN, VAR, np.zeros((F, K)), np.ones((F, K)), K, L,
                                         WS.astype(np.float32), objective_only=True)
        return ll, aux
    Edws, ll, aux = f.glm_step(y, None, lk.RR_LIK_GAUSSIAN, VAR, WS, K, L)
    return Edws, ll, aux, f.fm.glm_edphi(X.shape[0], 0, X.shape[1])


_REF_CACHE = {}


def _case_data(case):
    if case not in _REF_CACHE:
        rows, F, K, L = case
        X, y, WS = _exact_data(rows + F, rows, F, K * L)
        _REF_CACHE.clear()  # one case at a time (65 536 x 500 doubles each)
        _REF_CACHE[case] = (X, y, WS, _step_reference(X, y, WS, K, L))
    return _REF_CACHE[case]


# ---- tests --------------------------------------------------------------------------------------------------------------
def test_cases_cover_every_route():
    """The cases of this module, routed by the table at this device's CU count, reach every kernel of every product: the
    small, mid (always K-split: K >= 256 here) and 256 x 256 tile kernels, the tile kernel single-pass and K-split, the
    likelihood epilogue, the fused EdPhi contraction and the one-vector projection -- and a mid and a tile split whose last
    split is shorter than the others."""
    cu = _device().compute_units
    cases = route_cases(cu)
    want = {"fs": {"small", "mid_split", "tile", "tile_split", "lik"},
            "Ed": {"small", "mid_split", "tile", "tile_split"},
            "EdPhi": {"small", "mid_split", "tile", "tile_split", "gradt"},
            "project": {"rowvec", "small", "mid_split", "tile", "tile_split"}}
    hit = {p: {} for p in want}
    for label, p, r in cases:
        hit[p].setdefault(r[0], label)
    for p in want:
        for r in sorted(want[p]):
            print("%-8s %-11s %s" % (p, r, hit[p].get(r, "NOT HIT")))
    assert all(want[p] <= set(hit[p]) for p in want), {p: sorted(want[p] - set(hit[p])) for p in want}
    assert not any(r[0] == "mid" for _, _, r in cases)
    short = {r[0] for _, _, r in cases if r[0] in ("mid_split", "tile_split") and r[3] < r[2]}
    assert short == {"mid_split", "tile_split"}, short


@pytest.mark.parametrize("rows,F,S", PROJECT_CASES)
def test_project_is_exact_on_every_route(rows, F, S):
    """Phi W bit for bit: ragged rows, F and S off the 256 grid, S = 1 on the dot-product kernel."""
    X, _, _ = _exact_data(rows + F + S, rows, F, 1)
    W = _tern(np.random.RandomState(S), (F, S), 0.3)
    assert (np.abs(X) @ np.abs(W)).max() < EXACT
    f = _linear_features()
    try:
        out = f.project(X, [], W)
    finally:
        f.release()
    _assert_bitwise(out, X @ W, "project %s" % ((rows, F, S),))


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("case", STEP_CASES, ids=lambda c: "x".join(map(str, c)))
def test_step_is_exact_on_every_route(case, mode):
    """Edws = dfs Phi, the per-component sums of squares and log-likelihoods, and EdPhi = dfs^T ws / (K L) bit for bit, with
    the likelihood epilogue chosen by shape, forced and refused, and in deterministic mode (no mid kernel, no epilogue)."""
    rows, F, K, L = case
    X, y, WS, (Ed, ll, aux, EdPhi) = _case_data(case)
    f = _linear_features()
    try:
        with _Mode(mode):
            got = run_exact_step(f, X, y, WS, K, L)
    finally:
        f.release()
    for g, w, what in zip(got, (Ed, ll, aux, EdPhi), ("Edws", "llsum", "aux", "EdPhi")):
        _assert_bitwise(g, w, "%s %s %s" % (what, case, mode))


def test_step_sequence_is_exact():
    """ONE MinibatchFeatures through minibatches of changing size (P^T, dfs and dfs^T padded to 32-row, 256-row and max_rows
    extents; the transposing pass skipped or not), K L up and down (the scratch only grows, so later products run wider
    than their samples), a projection and an objective-only step in between: every step exact, so stale padding in any
    buffer shows up."""
    f = _linear_features()
    try:
        for i, (rows, K, L, what) in enumerate(SEQUENCE):
            if what == "project":
                X, _, _ = _exact_data(1000 + i, 700, SEQ_F, 1)
                W = _tern(np.random.RandomState(i), (SEQ_F, K), 0.3)
                _assert_bitwise(f.project(X, [], W), X @ W, "step %d: project" % i)
                continue
            X, y, WS = _exact_data(1000 + i, rows, SEQ_F, K * L)
            Ed, ll, aux, EdPhi = _step_reference(X, y, WS, K, L)
            if what == "objective":
                got, want, names = run_exact_step(f, X, y, WS, K, L, True), (ll, aux), ("llsum", "aux")
            else:
                got, want, names = run_exact_step(f, X, y, WS, K, L), (Ed, ll, aux, EdPhi), ("Edws", "llsum", "aux", "EdPhi")
            for g, w, n in zip(got, want, names):
                _assert_bitwise(g, w, "step %d %s: %s" % (i, (rows, K, L, what), n))
    finally:
        f.release()


def _rff_reference(X, y, W, ls, WS, K, L, chunk=2048):
    """Edws, llsum and the ARD length-scale gradients -(EdPhi o dPhi_i).sum() (glm.py:296-322, :274-275) of a Poisson (exp)
    step in float64, in row chunks (dPhi of 65 536 rows would take 8 GiB)."""
    from scipy.special import gammaln
    Ed = np.zeros((K * L, W.shape[1] * 2))
    ll = np.zeros(K)
    g = np.zeros(X.shape[1])
    for r0 in range(0, X.shape[0], chunk):
        Xc, yc = X[r0:r0 + chunk], y[r0:r0 + chunk]
        Phi = orc.rff_transform(Xc, W, ls)
        fs = WS @ Phi.T
        dfs = orc.lik_df("poisson_exp", yc, fs)
        Ed += dfs @ Phi
        # the step's sums leave out the constant -log(y!) (glm.py adds it once per minibatch)
        ll += (orc.lik_loglike("poisson_exp", yc, fs) + gammaln(yc + 1)).reshape(K, L, -1).sum(axis=(1, 2))
        EdPhi = dfs.T @ WS / (K * L)
        dP = orc.rff_grad(Xc, W, ls)
        g += np.einsum("rf,rfi->i", EdPhi, dP)
    return Ed, ll, -g


@pytest.mark.parametrize("rows", RFF_ROWS)
def test_config5_routes_with_random_fourier_features_vs_oracle(rows):
    """BASELINE config 5's product shapes (F = 2048, K L = 500) at 4352, 16 684 and 65 536 rows: the likelihood epilogue,
    the tile kernel's K-split for Ed and the fused EdPhi contraction, each picked by the shape alone, against the oracle."""
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd.btypes import Parameter, Positive
    cu = _device().compute_units
    K, L, n, d = RFF_K, RFF_L, RFF_N, RFF_D
    print(step_routes(rows, 2 * n, K * L, cu, lone_rff=True))
    rs = np.random.RandomState(rows)
    X = rs.randn(rows, d).astype(np.float32).astype(np.float64)
    y = rs.poisson(np.exp(0.4 * np.sin(X[:, 0]))).astype(float)
    basis = bs.RandomRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
    ls = np.linspace(0.8, 1.4, d)
    WS = 0.05 * rs.randn(K * L, 2 * n)
    f = bs.MinibatchFeatures(basis)
    try:
        f.assemble(X, [ls])
        Edws, ll, _ = f.glm_step(y, None, lk.RR_LIK_POISSON_EXP, 0.0, WS, K, L)
        g = np.asarray(f.glm_basis_grads(X), dtype=float)
    finally:
        f.release()
    Ed_ref, ll_ref, g_ref = _rff_reference(X, y, basis.W, ls, WS, K, L)
    assert normwise(Edws, Ed_ref) < 1e-3
    assert normwise(ll, ll_ref) < 1e-4
    assert g.shape == (d,) and normwise(g, g_ref) < 5e-3


# ---- which kernel ran (the bounds-checking build's launch counts; tests/test_debug_builds.py) ---------------------------
def census():
    """Launches of each GEMM kernel in one step (or projection) per case, under a library that counts them
    (rr_debug_kernel_launches): [(label, compute units, {kernel: launches}, {kernel: launches the table predicts})]."""
    import revrand_amd.basis_functions as bs
    from revrand_amd import likelihoods as lk
    from revrand_amd.btypes import Parameter, Positive
    dev = _device()
    lib, cu = dev.lib, dev.compute_units
    assert lib.rr_debug_kernel_launches(None) == 0

    def counts():
        dev.sync()
        return {k: int(lib.rr_debug_kernel_launches(k.encode())) for k in GEMM_KERNELS}

    def predicted(routes):
        want = dict.fromkeys(GEMM_KERNELS, 0)
        for r in routes:
            want[KERNEL[r[0]]] += 1
        return want

    out = []
    for rows, F, K, L in STEP_CASES:
        X, y, WS = _exact_data(rows + F, rows, F, K * L)
        for mode in MODES:
            f = _linear_features()
            try:
                with _Mode(mode):
                    f.assemble(X, [])
                    dev.sync()
                    lib.rr_debug_kernel_launches(None)
                    f.glm_step(y, None, lk.RR_LIK_GAUSSIAN, VAR, WS, K, L)
                    got = counts()
            finally:
                f.release()
            r = step_routes(rows, F, K * L, cu, det=mode == "det", fuse_lik=mode if mode in ("force", "0") else "auto")
            out.append(("step%s/%s" % ((rows, F, K, L), mode), cu, got, predicted(r.values())))
    for rows, F, S in PROJECT_CASES:
        X, _, _ = _exact_data(rows + F + S, rows, F, 1)
        f = _linear_features()
        try:
            f.assemble(X, [])
            dev.sync()
            lib.rr_debug_kernel_launches(None)
            f.fm.project(rows, np.ones((F, S)))
            got = counts()
        finally:
            f.release()
        out.append(("project%s" % ((rows, F, S),), cu, got, predicted([project_route(rows, F, S, cu)])))
    n, d, K, L = RFF_N, RFF_D, RFF_K, RFF_L
    basis = bs.RandomRBF(nbases=n, Xdim=d, random_state=1, lenscale=Parameter(np.ones(d), Positive()))
    ls = np.linspace(0.8, 1.4, d)
    for rows in RFF_ROWS:
        rs = np.random.RandomState(rows)
        X = rs.randn(rows, d)
        y = rs.poisson(1.0, size=rows).astype(float)
        WS = 0.05 * rs.randn(K * L, 2 * n)
        f = bs.MinibatchFeatures(basis)
        try:
            f.assemble(X, [ls])
            dev.sync()
            lib.rr_debug_kernel_launches(None)
            f.glm_step(y, None, lk.RR_LIK_POISSON_EXP, 0.0, WS, K, L)
            got = counts()
            f.glm_basis_grads(X)
        finally:
            f.release()
        out.append(("rff%d" % rows, cu, got, predicted(step_routes(rows, 2 * n, K * L, cu, lone_rff=True).values())))
    return out
