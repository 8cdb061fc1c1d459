"""The likelihood terms of the SVI step -- df = d loglike / d f and the log-likelihood term ll, per (row, weight sample) --
against float64 over their whole range: tails, the 1 + t == 1 switch of log1p, the underflow of exp(-|f|), large counts and a
large binomial n (tests/lik_cases.py: domain, grid, references, bound).

Three device implementations exist: rr_glm_lik_kernel (float32, after the first GEMM; RR_GLM_FUSE_LIK=0), the epilogue of
rr_gemm_lik_f32_kernel (float32; RR_GLM_FUSE_LIK=force) -- both through rr_lik_elem, rr_elbo.hip -- and rr_svi_lik (float64,
rr_svi_common.h) in the fused small-minibatch loop.

With X an identity matrix and K L a power of two the step's latent values are the weight samples themselves: the upload
scales by 1 / (K L), the product with a 1 is exact, the kernel scales back by K L.  Edws[kl][r] is then the single element
df[r][kl], whatever GEMM route ran (the other terms of its sum are exact zeros)."""
import numpy as np
import pytest

import lik_cases as lc
import revrand_oracle as orc
from test_gpu_glm_routes import _Mode, _linear_features

pytestmark = pytest.mark.gpu

MODES = ["0", "force"]   # the likelihood kernel behind the first GEMM / the epilogue of the first GEMM
ROUTE = {"0": "rr_glm_lik_kernel", "force": "rr_gemm_lik_f32_kernel"}


def _report(what, lik, mode, ratio):
    print("worst ratio to the bound: %-10s %-17s %-24s %.3g" % (what, lik, ROUTE.get(mode, mode), ratio))


def _describe(lik, what, y, n, f, got, want, ratio):
    return "%s %s: y=%g n=%g f=%r got=%r want=%r ratio to the bound=%.4g" % (lik, what, y, n, float(f), float(got), float(want), ratio)


# ---- A: per element ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("lik", lc.LIKS)
def test_every_grid_point_per_element(lik, mode):
    """One row, one feature, X = [[1]], K = 64, L = 1, the weight samples the grid: Edws[:, 0] is df and llsum[k] is ll of
    element k -- all 64 of each within the bound, for every target (and binomial n), with float32 and float64 targets (TY of
    rr_glm_lik_kernel, y_f64 of the epilogue), and llsum once more on the objective-only route (glm_step_draws with m the
    grid, C = 1e-12 and zero draws)."""
    grid = lc.grid(lik)
    lid, K = lc.LIK_ID[lik], 64
    X = np.ones((1, 1))
    WS = grid.astype(np.float64)[:, None]
    fails, top = [], {"df": 0.0, "ll": 0.0, "ll objective": 0.0}

    def check(what, got, want, S, y, n):
        i, r = lc.worst(got, want, lc.bound(grid, S))
        top[what] = max(top[what], r)
        if not r <= 1:
            fails.append(_describe(lik, what, y, n, grid[i], got[i], want[i], r))

    f = _linear_features()
    try:
        with _Mode(mode):
            for y, n in lc.targets(lik):
                ya, na = np.array([y]), np.array([n]) if lik == "binomial" else None
                want_df, want_ll = lc.ref_df(lik, y, grid, n), lc.ref_ll(lik, y, grid, n)
                S_df, S_ll = lc.s_df(lik, y, grid, n), lc.s_ll(lik, y, grid, n)
                for ytype in (np.float32, np.float64):
                    f.assemble(X, [])
                    if ytype is np.float32:
                        Edws, ll, _ = f.glm_step(ya, na, lid, 0.0, WS, K, 1)
                    else:
                        dy = f.dev.upload_vector(ya, np.float64)
                        dn = f.dev.upload_vector(na, np.float64) if na is not None else None
                        try:
                            Edws, ll, _ = f.fm.glm_step(dy, dn, lid, 0.0, WS, K, 1)
                        finally:
                            dy.free()
                            if dn is not None:
                                dn.free()
                    assert Edws.shape == (64, 1) and ll.shape == (64,)
                    check("df", Edws[:, 0], want_df, S_df, y, n)
                    check("ll", ll, want_ll, S_ll, y, n)
                f.assemble(X, [])
                _, _, ll, _ = f.glm_step_draws(ya, na, lid, 0.0, WS.T.copy(), np.full((1, K), 1e-12), K, 1,
                                               np.zeros((K, 1), dtype=np.float32), objective_only=True)
                check("ll objective", ll, want_ll, S_ll, y, n)
    finally:
        f.release()
    for what in sorted(top):
        _report(what, lik, mode, top[what])
    assert not fails, "%d of %d (target, output) pairs outside the bound; the worst element of each:\n%s" % (
        len(fails), 5 * len(lc.targets(lik)), "\n".join(fails))


# ---- B: in a tile --------------------------------------------------------------------------------------------------------
ROWS = 300
TILE_CASES = [(4, 8), (8, 64), (3, 7)]


def _tile_data(lik, K, L):
    """X = I_300; row r carries target r mod nt; component k takes its latent values from ONE band of the grid (a tail error is
    then not summed with terms of another magnitude): sample (k, l) of row r is value (r // nt + l) mod nb of the band.
    Returns y, n, WS (K L, 300) and the band of each component."""
    tg = lc.targets(lik)
    nt = len(tg)
    r = np.arange(ROWS)
    y = np.array([tg[i % nt][0] for i in r])
    n = np.array([tg[i % nt][1] for i in r])
    shift = 1 if K < 4 else 0   # three components: the two tails and the middle band
    WS = np.empty((K * L, ROWS))
    names = []
    for k in range(K):
        name = lc.BANDS[(k + shift) % 4]
        vals = lc.band(lik, name).astype(np.float64)
        names.append(name)
        for l in range(L):
            fi = (r // nt + l) % vals.size
            WS[k * L + l] = vals[fi]
            if l == 0:   # every (target, latent value) pair of the band occurs in this component
                assert len(set(zip((r % nt).tolist(), fi.tolist()))) == nt * vals.size, (lik, name)
    return y, n, WS, names


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("K,L", TILE_CASES, ids=lambda v: str(v))
@pytest.mark.parametrize("lik", lc.LIKS)
def test_tails_inside_a_tile(lik, K, L, mode):
    """X = I_300 (a partial 256-row tile; targets and the binomial's n change with the row), (K, L) = (4, 8), (8, 64) -- K L =
    512 crosses a 256-sample block of the likelihood kernel and a 256-column tile of the epilogue, with their per-component LDS
    sums -- and (3, 7): K L = 21 is no power of two, the kernel's f = fl(fl(ws / 21) 21) differs from the reference's f = ws
    by up to 2 ulp, which the 4 |f| of c(f) covers.

    df: per element, the bound of case A.  llsum[k] and EdPhi = dfs^T ws / (K L) are float32 sums: their bound is
    (max c + n_acc) EPS (sum of S over the summed elements) with n_acc the longest chain of float32 additions:
      llsum, epilogue: 64 fmas into red[j] (rr_gemm_lik_f32_kernel's tile loop, rr_elbo.hip:1331-1352), then one LDS atomic per
        lane that holds a column of the component (:1374): 4 lanes per column, at most min(L, 256) columns per tile;
        likelihood kernel: rows_per_block = 16 rows per thread (:1201-1210, glm_launch_lik :2243-2244), then min(L, 256) LDS
        atomics (:1216) -- the shorter chain.  Tiles / blocks are then added in float64.  n_acc = 64 + 4 min(L, 256).
      EdPhi: one dot product over the K L samples in float32 (fm_gemm; every route adds K L nonzero terms, in some order), of
        terms df ws / (K L) with ws / (K L) rounded to float32 once and df within c EPS S_df: n_acc = K L + 2."""
    y, n, WS, names = _tile_data(lik, K, L)
    lid, KL = lc.LIK_ID[lik], K * L
    X = np.eye(ROWS)
    fs = WS.T                                            # (rows, K L): what the oracle's X @ WS.T is
    want_df = lc.ref_df(lik, y[:, None], fs, n[:, None])
    S_df = lc.s_df(lik, y[:, None], fs, n[:, None])
    want_ll = lc.ref_ll(lik, y[:, None], fs, n[:, None])
    S_ll = lc.s_ll(lik, y[:, None], fs, n[:, None])
    f = _linear_features()
    try:
        with _Mode(mode):
            f.assemble(X, [])
            Edws, ll, _ = f.glm_step(y, n if lik == "binomial" else None, lid, 0.0, WS, K, L)
            EdPhi = f.fm.glm_edphi(ROWS, 0, ROWS)
    finally:
        f.release()
    assert Edws.shape == (KL, ROWS) and ll.shape == (K,) and EdPhi.shape == (ROWS, ROWS)
    # df, per element
    (r, kl), ratio = lc.worst(Edws.T, want_df, lc.bound(fs, S_df))
    _report("df", lik, mode, ratio)
    assert ratio <= 1, _describe(lik, "df (component %d: %s)" % (kl // L, names[kl // L]), y[r], n[r], fs[r, kl], Edws[kl, r],
                                 want_df[r, kl], ratio)
    # llsum, per component
    cmax = lc.c_of(fs).reshape(ROWS, K, L).max(axis=(0, 2))
    n_acc = 64 + 4 * min(L, 256)
    want = want_ll.reshape(ROWS, K, L).sum(axis=(0, 2))
    bnd = (cmax + n_acc) * lc.EPS * S_ll.reshape(ROWS, K, L).sum(axis=(0, 2)) + ROWS * L * lc.ABS_FLOOR
    (k,), ratio = lc.worst(ll, want, bnd)
    _report("llsum", lik, mode, ratio)
    assert ratio <= 1, "%s llsum[%d] (%s): got=%r want=%r ratio to the bound=%.4g" % (lik, k, names[k], ll[k], want[k], ratio)
    # EdPhi[r][c] = sum_kl df[r][kl] ws[kl][c] / (K L)
    Wn = WS / KL
    want = want_df @ Wn
    bnd = (lc.c_of(fs).max() + KL + 2) * lc.EPS * (S_df @ np.abs(Wn)) + KL * lc.ABS_FLOOR
    (r, c), ratio = lc.worst(EdPhi, want, bnd)
    _report("EdPhi", lik, mode, ratio)
    assert ratio <= 1, "%s EdPhi[%d][%d]: y=%g n=%g got=%r want=%r ratio to the bound=%.4g" % (lik, r, c, y[r], n[r], EdPhi[r, c],
                                                                                                want[r, c], ratio)


# ---- C: the fused float64 kernel -------------------------------------------------------------------------------------------
SVI_M, SVI_K, SVI_L = 20, 4, 2


@pytest.mark.parametrize("lik", lc.LIKS)
def test_fused_float64_kernel_over_the_range(lik):
    """rr_svi_lik (rr_svi_common.h:46) through one plain SGD step of the fused small-minibatch loop: one ("linear", M, False, I_M)
    child, M = 20 rows, K = 4 components, one band of the grid restricted to [-200, 40] per component, zero draws and C = 1e-12,
    so that w = m and f[j][k] = m[j][k]; target (j + s) mod nt on row j, one step per s: every (target, latent value) pair
    occurs.  (z0 - z1) / eta with eta = 1 is the gradient the kernel formed and objs[0] its -ELBO; against orc.glm_elbo, per
    element:  |diff| <= 1e-12 (|want| + B S_df) + 8 2^-53 |z0_i| / eta  (S_df on the coordinates of m, 0 elsewhere; the
    objective: B sum S_ll).  1e-12 leaves four orders over float64 rounding -- a wrong tail is an O(1) relative error -- and
    the second term is the cancellation in z0 - z1."""
    from revrand_amd import _hip
    M, K, L = SVI_M, SVI_K, SVI_L
    assert _hip.svi_supported_all(M, K, L, M, 1, M, 0, 0)
    grid = lc.grid(lik).astype(np.float64)
    grid = grid[(grid >= -200) & (grid <= 40)]
    m = np.empty((M, K))
    for k, name in enumerate(lc.BANDS):
        vals = lc.band(lik, name).astype(np.float64)
        vals = vals[vals <= 40]
        assert 3 <= vals.size <= M and set(vals.tolist()) <= set(grid.tolist())
        m[:, k] = np.resize(vals, M)
    assert set(m.ravel().tolist()) == set(grid.tolist())   # the whole restricted grid is there
    C = np.full((M, K), 1e-12)
    reg, eta, B = 1.0, 1.0, 1.0
    z0 = np.concatenate([m.ravel(), C.ravel(), [reg]])
    tg = lc.targets(lik)
    X = np.eye(M)
    e = np.zeros((K, L, M))
    dev = _hip.get_device()
    worst_g, worst_o = 0.0, 0.0
    for s in range(len(tg)):
        y = np.array([tg[(j + s) % len(tg)][0] for j in range(M)])
        n = np.array([tg[(j + s) % len(tg)][1] for j in range(M)])
        largs = (n,) if lik == "binomial" else ()
        bufs = [dev.upload_matrix(X), dev.upload_vector(y, np.float64), dev.upload_vector(lc.ll_constant(lik, y, n), np.float64),
                dev.upload_vector(np.arange(M), np.int32), dev.upload_vector(np.zeros((K * L, M)), np.float32)]
        if lik == "binomial":
            bufs.append(dev.upload_vector(n, np.float64))
        svi = None
        try:
            svi = _hip.FusedSvi(dev, [("linear", M, False, bufs[0])], M, bufs[1], bufs[5] if lik == "binomial" else None, bufs[2], K, L,
                                M, lc.LIK_ID[lik], 0, z0, np.full(z0.size, -np.inf), np.full(z0.size, np.inf),
                                np.zeros(z0.size, dtype=bool), _hip.UPDATER_IDS["SGDUpdater"], [eta], 1, B, all_children=True)
            svi.run(1, bufs[3], bufs[4])
            z1, objs, _ = svi.read()
        finally:
            if svi is not None:
                svi.close()
            for b in bufs:
                b.free()
        obj, (ndm, ndC, dL, _, _) = orc.glm_elbo(m, C, np.full(M, reg), [slice(0, M)], lik, [], largs, X, [], y, e, B)
        want = np.concatenate([ndm.ravel(), ndC.ravel(), np.ravel(dL)])
        got = (z0 - z1) / eta
        S = np.concatenate([lc.s_df(lik, y[:, None], m, n[:, None]).ravel(), np.zeros(M * K + 1)])
        bnd = 1e-12 * (np.abs(want) + B * S) + 8 * 2.0 ** -53 * np.abs(z0) / eta
        (i,), ratio = lc.worst(got, want, bnd)
        worst_g = max(worst_g, ratio)
        assert ratio <= 1, "%s shift %d: gradient coordinate %d (m[%d][%d] = %r, y = %g, n = %g): got=%r want=%r ratio=%.4g" % (
            lik, s, i, (i % (M * K)) // K, i % K, z0[i] if i < M * K else np.nan, y[(i % (M * K)) // K], n[(i % (M * K)) // K],
            got[i], want[i], ratio)
        S_obj = lc.s_ll(lik, y[:, None], m, n[:, None]).sum()
        _, ratio = lc.worst(objs[:1], [obj], 1e-12 * (abs(obj) + B * S_obj))
        worst_o = max(worst_o, ratio)
        assert ratio <= 1, "%s shift %d: objective got=%r want=%r ratio=%.4g" % (lik, s, objs[0], obj, ratio)
    _report("svi grad", lik, "svi_lik (float64)", worst_g)
    _report("svi obj", lik, "svi_lik (float64)", worst_o)
