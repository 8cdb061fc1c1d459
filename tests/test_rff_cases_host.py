"""Host checks of tests/rff_cases.py: its references against 50-digit arithmetic, its bounds against a NumPy emulation of
the kernels' projection (they admit correct code in any summation order and reject wrong code), and the coverage of its case
lists over the route table.  No GPU."""
import mpmath
import numpy as np
import pytest

import rff_cases as R

mpmath.mp.dps = 50
ORDERS = ("ascending", "even_odd", "pairwise")


def _unique(cases, with_arith=True):
    """One case per data set (and arithmetic): the references and bounds depend on nothing else."""
    seen, out = set(), []
    for c in cases:
        a = R.effective_arith(c.entry, c.compute)
        key = (c.family, c.rows, c.d, c.n, c.k, c.ard, c.seed, a if with_arith else (a == "f32"), c.entry.startswith("gm"))
        if key not in seen:
            seen.add(key)
            out.append(c)
    return out


ALL = R.all_cases()
# The sweeps below leave out the cases of a million rows and more (grid clamps, the longest tile walks, the sub-chunk seam): they
# draw from the same generators at the same d, n and k as their smaller neighbours, and their data sets assert their own
# exactness conditions when the GPU tests build them.  The coverage tests run over ALL.
DATA_CASES = _unique([c for c in ALL if not c.entry.startswith("gm") and not c.big])
GM_CASES = _unique([c for c in ALL if c.entry.startswith("gm")])


def _ids(cases):
    return [c.label for c in cases]


# ---- the references --------------------------------------------------------------------------------------------------------
def _mp_phase(D, c, r, f, mean_sign=0):
    li = np.broadcast_to(D.ls, (c.d,))
    if c.family == "A":   # the exact dyadic phase
        s = sum(int(D.X[r, i]) * int(D.Q[i, f]) for i in range(c.d))
        if mean_sign:
            s += mean_sign * sum(int(D.X[r, i]) * int(round(D.mean[i] / R.TWO_PI * 2 ** c.k)) for i in range(c.d))
        return mpmath.mpf(s % (1 << c.k)) / (1 << c.k)
    t = sum(mpmath.mpf(float(D.X[r, i])) * mpmath.mpf(float(D.W[i, f])) / (2 * mpmath.pi * mpmath.mpf(float(li[i]))) for i in range(c.d))
    if mean_sign:
        t += mean_sign * sum(mpmath.mpf(float(D.X[r, i])) * mpmath.mpf(float(D.mean[i])) / (2 * mpmath.pi) for i in range(c.d))
    return t


def _sample(c, k=5):
    rs = np.random.RandomState(c.rows + c.n)
    return [(int(rs.randint(c.rows)), int(rs.randint(c.n))) for _ in range(k)] + [(c.rows - 1, c.n - 1)]


@pytest.mark.parametrize("c", DATA_CASES, ids=_ids(DATA_CASES))
def test_references_agree_with_fifty_digit_arithmetic(c):
    """A sample of every data set: cos / sin of the reference phase, and the entries of the gradient built on them, to 1e-15."""
    D = R.case_data(c)
    n = c.n
    for r, f in _sample(c):
        t = _mp_phase(D, c, r, f)
        for blk, fn in ((0, mpmath.cos), (1, mpmath.sin)):
            want = fn(2 * mpmath.pi * t)
            assert abs(mpmath.mpf(float(D.want[r, blk * n + f])) - want) < 1e-15, (c.label, r, f, blk)
        assert abs(float(D.A[r, f])) >= abs(float(D.phase[r, f])) * (1 - 1e-12)
    if c.entry == "grad":
        want, adz = R.grad_reference(D, c)
        li = np.broadcast_to(D.ls, (c.d,))
        for r, f in _sample(c, 3):
            t = _mp_phase(D, c, r, f)
            for i in range(want.shape[2]):
                dz = -mpmath.mpf(float(D.X[r, i])) * mpmath.mpf(float(D.W[i, f])) / mpmath.mpf(float(li[i])) ** 2
                assert abs(mpmath.mpf(float(want[r, f, i])) + mpmath.sin(2 * mpmath.pi * t) * dz) <= 1e-15 * max(1, abs(dz))
                assert abs(mpmath.mpf(float(want[r, n + f, i])) - mpmath.cos(2 * mpmath.pi * t) * dz) <= 1e-15 * max(1, abs(dz))
                assert abs(float(adz[r, f, i]) - abs(dz)) <= 1e-15 * max(1, abs(dz))


@pytest.mark.parametrize("c", GM_CASES, ids=_ids(GM_CASES))
def test_spectral_mixture_references_agree_with_fifty_digit_arithmetic(c):
    D = R.gm_data(c)
    n = c.n
    for r, f in _sample(c, 3):
        for j, sgn in ((0, 1), (2, -1)):
            t = _mp_phase(D, c, r, f, sgn)
            assert abs(mpmath.mpf(float(D.want4[r, j * n + f])) - mpmath.cos(2 * mpmath.pi * t)) < 1e-15, (c.label, r, f, j)
            assert abs(mpmath.mpf(float(D.want4[r, (j + 1) * n + f])) - mpmath.sin(2 * mpmath.pi * t)) < 1e-15, (c.label, r, f, j)


def test_the_librarys_literals_are_the_ones_restated_here():
    """inv2pi and twopi as rr_api.hip spells them, to the last digit the sources carry."""
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "revrand_amd", "csrc", "rr_api.hip")).read()
    assert "inv2pi = 0.15915494309189533576888" in src and "twopi = 6.283185307179586476925" in src
    assert abs(mpmath.mpf(R.INV2PI) * 2 * mpmath.pi - 1) < 2.0 ** -53


# ---- the bounds admit correct code and reject wrong code ---------------------------------------------------------------------
EMULATED_ROWS = 4096   # of a data set of more rows (the grid-clamp and tile-walk cases) the first 4096: rows are drawn alike


def _chunks(c):
    rows = min(c.rows, EMULATED_ROWS)
    step = max(1, (1 << 22) // (c.d * c.n))
    return [(r0, min(rows, r0 + step)) for r0 in range(0, rows, step)]


def _emulated_ratio(c, D, arith, order, mutant=None, odt=None):
    """The NumPy emulation in `arith` against the bound of that arithmetic (output type odt, the case's by default): (largest
    ratio over all elements, fraction of the touched elements beyond their bound, largest |error|)."""
    worst, beyond, touched, emax = 0.0, 0, 0, 0.0
    for r0, r1 in _chunks(c):
        sub = R.SimpleNamespace(X=D.X[r0:r1], W=D.W, ls=D.ls)
        got, mask = R.emulate(sub, arith, order, mutant)
        err = np.abs(got - D.want[r0:r1]).astype(np.float64)
        bound = R.phi_bound(arith, odt or c.odt, c.family, c.d, D.A[r0:r1], c.n)
        ratio = err / bound
        worst = max(worst, float(ratio.max()))
        beyond += int((ratio[mask] > 1).sum())
        touched += int(mask.sum())
        emax = max(emax, float(err.max()))
    return worst, beyond / max(touched, 1), emax


def _emul_arith(c):
    return "f32" if R.effective_arith(c.entry, c.compute) == "f32" else "f64"


@pytest.mark.parametrize("c", DATA_CASES, ids=_ids(DATA_CASES))
def test_bound_admits_the_projection_in_any_summation_order(c):
    """The emulated projection -- Ws and x rounded to the type, a rounding after every product and every add, ascending,
    even-then-odd and pairwise -- with float64 sine / cosine.  Family B: the float32 emulation stays below one half of the
    float32 bound on every data set, whatever arithmetic the case itself runs in.  In the case's own arithmetic it stays below
    the bound: float32 on family A is exact (what is left is this emulation's float64 cosine); in float64 the table's own
    error -- two roundings, 1.6 u measured on family A -- and the roundings of the sum share a budget of (d + 2) u, of which
    correct code uses two thirds at d = 1, so the line there is the bound itself."""
    D = R.case_data(c)
    arith = _emul_arith(c)
    for order in ORDERS:
        if c.family == "B":
            worst = _emulated_ratio(c, D, "f32", order, odt="f32")[0]
            assert worst < 0.5, (c.label, order, worst)
        worst = _emulated_ratio(c, D, arith, order, odt="f64" if arith == "f64" else None)[0]
        assert worst < (1e-6 if (c.family, arith) == ("A", "f32") else 1.0), (c.label, order, worst)


def _mutants(c):
    for m in R.MUTANTS:
        if m == "inv2pi_1e-12" and _emul_arith(c) != "f64":
            continue   # float64 arithmetic only: 5.6e-12 relative is far below float32's own rounding
        yield m


MUTANT_CASES = [c for c in DATA_CASES if c.family == "A" or c.d <= 32]


@pytest.mark.parametrize("c", MUTANT_CASES, ids=_ids(MUTANT_CASES))
def test_bound_rejects_wrong_code(c):
    """Mutants of the emulation exceed the bound on more than half of the elements they touch (both blocks for a dropped
    dimension, a coarser x and a truncated 1 / 2 pi; the sine block for its flipped sign; the first 32 frequencies of both
    blocks for the swap), on every family-A data set and every family-B one with d <= 32.  x rounded to ten mantissa bits is
    the identity on family A's integers of at most four bits -- asserted, and the mutant held on family B alone.  The truncated
    1 / 2 pi (float64 arithmetic and output: a float32 store hides it behind 2^-24) stays inside the old tolerances -- 1e-9
    normwise at a revolution or two, family B; 1e-5 at family A's tens of revolutions: only a per-element bound sees it."""
    D = R.case_data(c)
    arith = _emul_arith(c)
    for m in _mutants(c):
        if m == "x_10bit" and c.family == "A":
            assert np.array_equal(R.round_mantissa(D.X, 10), D.X)
            continue
        worst, frac, emax = _emulated_ratio(c, D, arith, "ascending", m, odt="f64" if arith == "f64" else None)
        assert frac > 0.5, (c.label, m, frac, worst)
        if m == "inv2pi_1e-12":
            assert emax < (1e-9 if c.family == "B" else 1e-5), (c.label, emax)


def test_mutant_rates_on_gaussian_data_match_the_recorded_ones():
    """The guide figures of the issue on the family-B data of this module: a dropped last dimension is caught on 99.9 % or
    more of the elements, ten mantissa bits of x on 85 % or more, at d = 1, 8, 32."""
    for d in (1, 8, 32):
        c = R.case("rates/d=%d" % d, "transform_dev", "f32", 64, d, 64, family="B", seed=d)
        D = R.case_data(c)
        assert _emulated_ratio(c, D, "f32", "ascending", "drop_last_dim")[1] >= 0.999
        assert _emulated_ratio(c, D, "f32", "ascending", "x_10bit")[1] >= 0.85
        assert _emulated_ratio(c, D, "f32", "pairwise")[0] < 0.5


# ---- coverage --------------------------------------------------------------------------------------------------------------
def _rows_at(cu):
    rows, grids = set(), []
    for c in ALL:
        r = R.case_route(c, cu)
        assert r.error is None, (c.label, r.error)
        rows |= set(r.rows)
        grids += [(c.label,) + g for g in r.grids]
    return rows, grids


def test_cases_reach_every_row_of_the_route_table_at_256_compute_units():
    rows, grids = _rows_at(256)

    def have(prefix, *parts):
        return any(r.startswith(prefix) and all(p in r.split("/") for p in parts) for r in rows)

    pairs = [("f32", "f32"), ("f32", "f64"), ("f64", "f32"), ("f64", "f64")]
    for dm in R.DMAXES:
        D = "DMAX=%d" % dm
        assert have("mfma/", D) and have("mfma64/", D), dm
        for arith in ("f32", "f64"):
            assert have("valu_transform/", D, arith), (dm, arith)
            assert have("valu_grad/", D, arith), (dm, arith)
            assert have("valu_features/", D, arith), (dm, arith)
            assert have("gm_transform/", D, arith) and have("gm_grad/", D, arith), (dm, arith)
        assert have("mfma/", D, "has_y") and have("mfma/", D, "wt") and have("mfma/", D, "plain"), dm
        assert have("mfma64/", D, "has_y") and have("mfma64/", D, "plain"), dm
        assert have("mfma64/", D, "f32->f32") or have("mfma64/", D, "f64->f32"), dm   # the float32-output (RR_F32P64) use
    for x, o in pairs:
        p = "%s->%s" % (x, o)
        assert have("mfma/", p) and have("mfma64/", p), p
        assert any(r.startswith("valu_transform/") and r.split("/")[2] == x and r.split("/")[4] == o for r in rows), p
        assert any(r.startswith("valu_grad/") and r.split("/")[2] == x and r.split("/")[4] == o for r in rows), p
    for x in ("f32", "f64"):
        assert have("mfma/", "%s->f32" % x, "has_y") and have("mfma/", "%s->f32" % x, "wt")
        assert have("mfma64/", "%s->f64" % x, "has_y") and have("mfma64/", "%s->f32" % x, "has_y")
        assert have("valu_features/", x, "has_y") and have("valu_features/", x, "plain")
    assert have("valu_features/", "f64", "lds") and have("valu_transform/", "f64", "lds")
    assert "mfma/deterministic" in rows and "mfma64/deterministic" in rows
    # the three shapes of the Xdim > 128 route, with and without targets, and its gradient
    for r in ("large/gemm_trig/f32->f32", "large/gemm_trig/f64->f32", "large/gemm_trig/f32->f32/has_y", "large/gemm+trig/f64->f64",
              "large/phase64+trig/f64->f64", "large/phase64+trig/f32->f32", "large/phase64+trig/f64->f64/has_y", "large/trig/f32/f64",
              "large/trig/f64/f64", "large/trig/f64/f32", "large/grad_p/f32/f32/f32", "large/grad_p/f64/f64/f64", "large/xt/f32", "large/xt/f64"):
        assert r in rows, r
    assert {"prepare/kernel", "prepare/host", "prepare/dev"} <= rows
    # both GEMM kernels of the float64-output shape, and more than one sub-chunk
    seam = R.case_route([c for c in ALL if c.label == "L/t/f32->f64/seam"][0], 256)
    assert seam.kernels["rr_gemm_tn_f32_kernel"] == 1 and seam.kernels["rr_gemm_tn_small_f32_kernel"] == 1 and seam.kernels["rr_trig_kernel"] == 2
    assert R.case_route([c for c in ALL if c.label == "L/t/f32/seam"][0], 256).kernels["rr_gemm_trig_f32_kernel"] == 2
    assert R.case_route([c for c in ALL if c.label == "L/t/f64/seam"][0], 256).kernels["rr_phase_f64_kernel"] == 2
    # tiles per workgroup: every value the halving reaches, the override and the clamp
    tpb = {g[4] for g in grids if g[1] == "rr_rff_features_mfma_kernel"}
    assert {2, 3, 4, 8, 16, 32, 64} <= tpb, sorted(tpb)
    assert {4, 8, 16} <= {g[4] for g in grids if g[1] == "rr_rff_features_mfma64_kernel"}
    clamp = R.case_route(R.CLAMP_MFMA, 256).grids[0]
    assert clamp[1:] == (1, 32769, 2)   # 65537 tiles at one per workgroup would be 65537 row blocks: two per workgroup
    g = R.case_route(R.CLAMP_VALU_G, 256).grids[0]
    assert g == ("rr_rff_grad_kernel", 1, 61681, 17)
    t = R.case_route(R.CLAMP_VALU_T, 256).grids[0]
    assert t[0] == "rr_rff_transform_kernel" and t[2] <= 65535   # (its clamp is unreachable below 4096 CUs: R.UNREACHABLE)
    # remainder rows go to the VALU kernel while the body of the same call runs on the matrix cores
    both = [c for c in ALL if c.entry == "transform_dev" and {"rr_rff_transform_kernel"} < set(R.case_route(c, 256).kernels)]
    assert len(both) > 40
    # misaligned rows take the VALU kernels for the whole call
    for c in R.align_cases():
        k = R.case_route(c, 256).kernels
        assert k["rr_rff_features_mfma_kernel"] == 0 and k["rr_rff_features_mfma64_kernel"] == 0, c.label
    assert len(R.UNREACHABLE) == 5 and all(len(v) > 40 for v in R.UNREACHABLE.values())


@pytest.mark.parametrize("cu", [1, 8, 64, 104, 228, 256, 304, 4096])
def test_every_case_resolves_to_a_route_at_any_cu_count(cu):
    for c in ALL:
        r = R.case_route(c, cu)
        assert r.error is None and sum(r.kernels.values()) >= 1, (c.label, cu)
        for g in r.grids:
            assert 1 <= g[2] <= 65535 and g[1] >= 1, (c.label, cu, g)


def test_a_float64_phase_basis_with_misaligned_rows_is_refused():
    for entry in ("gram", "put_rff"):
        r = R.feature_route(entry, "f32p64", "f64", "f32", 70, 9, 33, ldx_bytes=17 * 8)
        assert r.error and not r.kernels["rr_rff_features_mfma64_kernel"]
        r = R.feature_route(entry, "f32p64", "f64", "f32", 70, 9, 33, env={"RR_FEATURES_NO_MFMA64": "1"})
        assert r.error


def test_route_examples():
    """A few routes worked out by hand from the launchers."""
    r = R.feature_route("transform_dev", "f32", "f32", "f32", 33, 9, 33)
    assert r.counts() == dict(R.Route().counts(), rr_scale_w_kernel=1, rr_rff_features_mfma_kernel=1, rr_rff_transform_kernel=1)
    r = R.feature_route("transform_dev", "f64", "f64", "f64", 15, 9, 33)
    assert r.counts() == dict(R.Route().counts(), rr_scale_w_kernel=1, rr_rff_transform_kernel=1)
    r = R.feature_route("transform_dev", "f32p64", "f64", "f32", 16, 9, 33)
    assert r.counts() == dict(R.Route().counts(), rr_scale_w_kernel=1, rr_rff_features_mfma64_kernel=1)
    r = R.feature_route("gram", "f32", "f32", "f64", 70, 200, 17, with_y=True)
    assert r.counts() == dict(R.Route().counts(), rr_xt_kernel=1, rr_gemm_trig_f32_kernel=1)
    r = R.feature_route("grad", "f64", "f64", "f64", 9, 129, 17)
    assert r.counts() == dict(R.Route().counts(), rr_phase_f64_kernel=1, rr_trig_kernel=1, rr_rff_grad_p_kernel=1)
    r = R.feature_route("put_gm", "f32", "f32", "f32", 70, 9, 33)
    assert r.counts() == dict(R.Route().counts(), rr_scale_w_dev_kernel=2, rr_rff_features_mfma_kernel=2)
    assert R.mfma_grid(32 * 9000, 8, 8, 256, {}) == (1, 563, 16) and R.mfma_grid(64, 8, 8, 256, {}) == (1, 1, 4)
    assert R.mfma_grid(32 * 9000, 8, 8, 104, {})[2] == 16 and R.mfma_grid(32 * 9000, 8, 8, 32, {})[2] == 64
