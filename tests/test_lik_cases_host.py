"""tests/lik_cases.py checked on the host: its grid, its float64 references against 50-digit arithmetic, and that its bound is
one correct float32 code can meet with room for the hardware's exp2 / log2 / rcp."""
import numpy as np
import pytest

import lik_cases as lc
import revrand_oracle as orc

CASES = [(lik, y, n) for lik in lc.LIKS for y, n in lc.targets(lik)]


def test_the_grids_hold_the_named_points():
    """64 distinct float32 values each; 0 and both signs of every named magnitude (the exp link: the positive ones up to 80,
    the rest replaced inside (17, 80]); everything inside the domain; every band of test B non-empty and disjoint."""
    for lik in lc.LIKS:
        g = lc.grid(lik)
        assert g.dtype == np.float32 and g.shape == (64,) and np.unique(g).size == 64
        assert np.all(lc.in_domain(lik, g))
        have = set(g.tolist())
        assert 0.0 in have
        for v in lc.NAMED:
            v32 = float(np.float32(v))
            assert -v32 in have, (lik, -v)
            assert (v32 in have) == (lik != "poisson_exp" or v <= 80), (lik, v)
        if lik == "poisson_exp":
            assert g.max() == 80 and np.sum((g > 17) & (g <= 80)) == 5 + 11
        bands = [lc.band(lik, b) for b in lc.BANDS]
        assert all(b.size >= 5 for b in bands) and sum(b.size for b in bands) == 64
    assert not np.array_equal(lc.GRID, lc.GRID_EXP)
    # the switch of log1p at 1 + t == 1 and exp's underflow lie between grid points
    t = np.exp(-np.abs(lc.GRID.astype(np.float64))).astype(np.float32)
    one = np.float32(1) + t == np.float32(1)
    assert one[np.abs(lc.GRID) >= 17].all() and not one[np.abs(lc.GRID) <= 16.6].any()
    assert np.sum(t == 0) >= 4 and np.sum((t > 0) & (t < np.float32(2.0 ** -126))) >= 8


def test_the_likelihood_ids_are_the_package_s():
    from revrand_amd import likelihoods as lk
    assert lc.LIK_ID == {"bernoulli": lk.RR_LIK_BERNOULLI, "binomial": lk.RR_LIK_BINOMIAL, "gaussian": lk.RR_LIK_GAUSSIAN,
                         "poisson_exp": lk.RR_LIK_POISSON_EXP, "poisson_softplus": lk.RR_LIK_POISSON_SOFTPLUS}


def test_the_targets_are_the_issue_s():
    assert lc.targets("bernoulli") == [(0.0, 1.0), (1.0, 1.0)]
    assert [y for y, _ in lc.targets("poisson_softplus")] == [0, 1, 2, 7, 35, 1000, 100000]
    assert lc.targets("poisson_exp") == lc.targets("poisson_softplus")
    assert sorted(lc.BINOMIAL_NY) == [(0, 0), (1, 0), (1, 1), (8, 0), (8, 1), (8, 3), (8, 4), (8, 8), (1000, 0), (1000, 1),
                                      (1000, 3), (1000, 500), (1000, 1000)]


@pytest.mark.parametrize("lik", lc.LIKS)
def test_ref_ll_is_lik_loglike_without_its_constants(lik):
    """ref_ll + the gammaln terms == the oracle's lik_loglike, to the rounding of those terms"""
    f = lc.grid(lik).astype(float)
    for y, n in lc.targets(lik):
        args = (n,) if lik == "binomial" else ()
        full = orc.lik_loglike(lik, y, f, *args)
        const = lc.ll_constant(lik, y, n)
        mine = lc.ref_ll(lik, y, f, n)
        assert np.all(np.abs(mine + const - full) <= 4 * 2.0 ** -53 * (np.abs(mine) + np.abs(const) + 1e-300)), (lik, y, n)


def _mp_terms(mp, lik, y, f, n):
    """(df, ll) at 50 digits: the exact function, no clamp"""
    f, y, n = mp.mpf(float(f)), mp.mpf(float(y)), mp.mpf(float(n))
    sp = mp.log1p(mp.exp(f)) if f < 0 else f + mp.log1p(mp.exp(-f))
    ex = 1 / (1 + mp.exp(-f))
    if lik in ("bernoulli", "binomial"):
        nn = n if lik == "binomial" else mp.mpf(1)
        return y - nn * ex, y * f - nn * sp
    if lik == "poisson_exp":
        return y - mp.exp(f), y * f - mp.exp(f)
    return ex * (y / sp - 1), y * mp.log(sp) - sp


@pytest.mark.parametrize("lik", lc.LIKS)
def test_the_float64_references_against_50_digits(lik):
    """|oracle - exact| <= 64 2^-53 S on every (y, n, f) of the grid: the yardstick is six decimal orders finer than the
    float32 bound it is used in"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    f = lc.grid(lik)
    worst = 0.0
    for y, n in lc.targets(lik):
        df, ll = lc.ref_df(lik, y, f, n), lc.ref_ll(lik, y, f, n)
        sd, sl = lc.s_df(lik, y, f, n), lc.s_ll(lik, y, f, n)
        for i, fi in enumerate(f):
            wdf, wll = _mp_terms(mp, lik, y, fi, n)
            for got, want, S, what in ((df[i], wdf, sd[i], "df"), (ll[i], wll, sl[i], "ll")):
                err = float(abs(mp.mpf(float(got)) - want))
                lim = 64 * 2.0 ** -53 * float(S)
                worst = max(worst, err / lim if lim > 0 else (0.0 if err == 0 else np.inf))
                assert err <= lim, (lik, what, y, n, float(fi), float(got), float(want), err / lim if lim else np.inf)
    print("%s: worst |oracle - exact| / (64 2^-53 S) = %.3f" % (lik, worst))


@pytest.mark.parametrize("lik,y,n", CASES, ids=lambda v: str(v))
def test_correct_float32_code_stays_below_a_quarter_of_the_bound(lik, y, n):
    """The device formulas restated in numpy float32 (correctly rounded exp / log / division): at most 0.25 of the bound on
    every grid point, which leaves a factor of 4 for the hardware's approximate exp2, log2 and reciprocal."""
    f = lc.grid(lik)
    df, ll = lc.emulate_f32(lik, y, f, n)
    assert df.dtype == np.float32 and ll.dtype == np.float32 and np.all(np.isfinite(df)) and np.all(np.isfinite(ll))
    for got, want, S, what in ((df, lc.ref_df(lik, y, f, n), lc.s_df(lik, y, f, n), "df"),
                               (ll, lc.ref_ll(lik, y, f, n), lc.s_ll(lik, y, f, n), "ll")):
        i, r = lc.worst(got, want, lc.bound(f, S))
        assert r <= 0.25, (lik, what, y, n, float(f[i]), float(got[i]), float(want[i]), r)


def test_the_clamped_poisson_softplus_formula_misses_the_bound_in_the_tail():
    """What the rewrite of the Poisson-softplus element removed: with g clamped at 1e-37 and divided by, df is 0 instead of ~y
    once exp(f) is 0, infinite when y / g overflows, NaN (0 x inf) when y >= 35 meets the clamp; ll is y log(1e-37) instead of
    y f.  The bound notices each of them -- and passes the old formula wherever it was right (|f| <= 80, y <= 1000)."""
    lik = "poisson_softplus"
    f = lc.GRID
    with np.errstate(all="ignore"):
        df, ll = lc.emulate_f32(lik, 1.0, f, fixed=False)
        lo = int(np.where(f == np.float32(-104))[0][0])   # exp(-104) is 0 in float32, flushed or not
        assert df[lo] == 0 and abs(lc.ref_df(lik, 1.0, f)[lo] - 1) < 1e-6
        assert abs(ll[lo] - np.log(1e-37)) < 1e-3 and abs(lc.ref_ll(lik, 1.0, f)[lo] + 104) < 1e-6
        i80 = int(np.where(f == np.float32(-80))[0][0])
        assert np.isinf(lc.emulate_f32(lik, 1e5, f, fixed=False)[0][i80]) and np.isfinite(lc.ref_df(lik, 1e5, f)[i80])
        assert np.isnan(lc.emulate_f32(lik, 35.0, f, fixed=False)[0]).any()
        for y in (1.0, 35.0, 1e5):
            got = lc.emulate_f32(lik, y, f, fixed=False)
            assert lc.worst(got[0], lc.ref_df(lik, y, f), lc.bound(f, lc.s_df(lik, y, f)))[1] > 1e3
            assert lc.worst(got[1], lc.ref_ll(lik, y, f), lc.bound(f, lc.s_ll(lik, y, f)))[1] > 1e3
        ok = np.abs(f) <= 80
        for y in (0.0, 1.0, 2.0, 7.0, 35.0, 1000.0):
            got = lc.emulate_f32(lik, y, f[ok], fixed=False)
            assert lc.worst(got[0], lc.ref_df(lik, y, f[ok]), lc.bound(f[ok], lc.s_df(lik, y, f[ok])))[1] <= 0.25
            assert lc.worst(got[1], lc.ref_ll(lik, y, f[ok]), lc.bound(f[ok], lc.s_ll(lik, y, f[ok])))[1] <= 0.25


def test_flushing_subnormal_exponentials_would_miss_the_bound_for_a_large_binomial_n():
    """Why rr_expneg (rr_elbo.hip) scales its argument: exp2 on the device returns 0 below 2^-126, and n exp(f) with n = 1000
    is 6e-36 at f = -88 -- six times the absolute floor of the bound."""
    f = lc.GRID
    df, _ = lc.emulate_f32("binomial", 0.0, f, 1000.0, flush=True)
    assert lc.worst(df, lc.ref_df("binomial", 0.0, f, 1000.0), lc.bound(f, lc.s_df("binomial", 0.0, f, 1000.0)))[1] > 1
