"""The latent values, targets, float64 references and error bound that hold the per-element likelihood terms of the SVI
step -- df = d loglike / d f and the f-dependent part ll of loglike -- over their whole range (pure numpy; shared by
tests/test_lik_cases_host.py and tests/test_gpu_lik_tails.py).

Domain: finite float32 f in [-200, 200] ([-200, 80] for the exp link, whose mean overflows float32 at f = 88.7); Bernoulli
y in {0, 1}; Poisson y in POISSON_Y; binomial (n, y) in BINOMIAL_NY.

References: the oracle's lik_df, and lik_loglike without the f-independent gammaln constants the host adds once per
minibatch (restated from the oracle's own softplus: subtracting gammaln(1e5 + 1) ~ 1e6 from a term of size 1 would cost the
reference ten digits; tests/test_lik_cases_host.py checks the restatement against lik_loglike and both against mpmath).  The
oracle's softplus is deliberately NOT the reference project's logsumexp([0, f]), which rounds to 0 below f = -37: it is the
exact function in its log1p form.

Bound: |got - ref| <= c(f) EPS S + 1e-36 with EPS = 2^-24, c(f) = 16 + 4 |f| and S the sum of the absolute values of the
formula's terms, in float64 (`bound`).  16: at most eight float32 operations at up to 2 ulp each; 4 |f|: an error of a few
ulp of f -- the argument of exp is rounded in exp2(f log2 e), and f itself was formed from ws / (K L) in float32 -- moves
exp(f) by that many ulp times |f|.  1e-36: results below float32's normal range may be flushed to zero.

    likelihood                      S_df                        S_ll
    Bernoulli (n = 1) / binomial    |y| + n expit(f)            |y f| + n softplus(f)
    Poisson, exp link               |y| + exp(f)                |y f| + exp(f)
    Poisson, softplus link          expit(f) (y / g + 1)        |y log g| + g          (g = softplus(f))
"""
import numpy as np

import revrand_oracle as orc

EPS = 2.0 ** -24
ABS_FLOOR = 1e-36
LIKS = ("bernoulli", "binomial", "poisson_exp", "poisson_softplus")
LIK_ID = {"bernoulli": 0, "binomial": 1, "gaussian": 2, "poisson_exp": 3, "poisson_softplus": 4}   # include/revrand_hip.h

BERNOULLI_Y = (0.0, 1.0)
POISSON_Y = (0.0, 1.0, 2.0, 7.0, 35.0, 1000.0, 100000.0)
BINOMIAL_NY = tuple((float(n), float(y)) for n in (0, 1, 8, 1000) for y in sorted({0, 1, 3, n // 2, n}) if y <= n)

# the magnitudes every grid holds with both signs: around 0, the 1 + t == 1 switch of log1p(t) at |f| = 24 ln 2 = 16.6, the
# float32 underflow of exp(-|f|) (normal down to 87.3, subnormal down to 103.3), the ends of the domain
NAMED = (1e-30, 1e-8, 1e-3, 0.25, 0.5, 1, 2, 3.3, 5, 8, 12, 16, 16.6, 17, 20, 30, 40, 60, 80, 86, 87, 87.3, 88, 90, 95, 100,
         103, 104, 120, 200)
# filled to 64: 24 ln 2 on both sides, and -37, below which logsumexp([0, f]) returns 0
FILL = (-16.635532, 16.635532, -37.0)
# the exp link's domain ends at 80: its eleven positive values above 80 are replaced by values in (17, 80]
EXP_FILL = (18, 22, 25, 35, 45, 50, 55, 65, 70, 75, 79.5)


def _grid(exp_link):
    pos = [v for v in NAMED if not (exp_link and v > 80)] + (list(EXP_FILL) if exp_link else [])
    g = np.array([0.0] + pos + [-v for v in NAMED] + list(FILL), dtype=np.float32)
    assert g.size == 64 and np.unique(g).size == 64
    return g


GRID = _grid(False)
GRID_EXP = _grid(True)


def grid(lik):
    """The 64 float32 latent values of a likelihood"""
    return GRID_EXP if lik == "poisson_exp" else GRID


def in_domain(lik, f):
    f = np.asarray(f, dtype=float)
    return np.isfinite(f) & (f >= -200) & (f <= (80 if lik == "poisson_exp" else 200))


def targets(lik):
    """[(y, n)] of a likelihood (n: the binomial's count, 1 for Bernoulli, unused by the Poissons)"""
    if lik == "bernoulli":
        return [(y, 1.0) for y in BERNOULLI_Y]
    if lik == "binomial":
        return [(y, n) for n, y in BINOMIAL_NY]
    return [(y, 0.0) for y in POISSON_Y]


BANDS = ("centre", "middle", "low", "high")


def band(lik, which):
    """The grid's values with |f| <= 1 / 1 < |f| <= 17 / f < -17 / f > 17: terms of one magnitude"""
    g = grid(lik).astype(float)
    sel = {"centre": np.abs(g) <= 1, "middle": (np.abs(g) > 1) & (np.abs(g) <= 17), "low": g < -17, "high": g > 17}[which]
    return grid(lik)[sel]


def c_of(f):
    return 16.0 + 4.0 * np.abs(np.asarray(f, dtype=float))


def _args(lik, n):
    return (n,) if lik == "binomial" else ()


def ref_df(lik, y, f, n=1.0):
    return orc.lik_df(lik, y, np.asarray(f, dtype=float), *_args(lik, n))


def ref_ll(lik, y, f, n=1.0):
    """lik_loglike (oracle/revrand_oracle.py:431-448) without its gammaln terms"""
    y, f, n = np.broadcast_arrays(np.asarray(y, float), np.asarray(f, float), np.asarray(n, float))
    if lik == "bernoulli":
        return y * f - orc.softplus(f)
    if lik == "binomial":
        return y * f - n * orc.softplus(f)
    if lik == "poisson_exp":
        return y * f - np.exp(f)
    if lik == "poisson_softplus":
        g = orc.softplus(f)
        return y * np.log(g) - g
    raise ValueError(lik)


def ll_constant(lik, y, n=1.0):
    """What lik_loglike adds to ref_ll: a function of the targets alone"""
    from scipy.special import gammaln
    y, n = np.broadcast_arrays(np.asarray(y, float), np.asarray(n, float))
    if lik == "bernoulli":
        return np.zeros(y.shape)
    if lik == "binomial":
        return gammaln(n + 1) - gammaln(y + 1) - gammaln(n - y + 1)
    return -gammaln(y + 1)


def s_df(lik, y, f, n=1.0):
    y, f, n = np.broadcast_arrays(np.asarray(y, float), np.asarray(f, float), np.asarray(n, float))
    if lik in ("bernoulli", "binomial"):
        return np.abs(y) + (n if lik == "binomial" else 1.0) * orc._expit(f)
    if lik == "poisson_exp":
        return np.abs(y) + np.exp(f)
    return orc._expit(f) * (y / orc.softplus(f) + 1.0)


def s_ll(lik, y, f, n=1.0):
    y, f, n = np.broadcast_arrays(np.asarray(y, float), np.asarray(f, float), np.asarray(n, float))
    if lik in ("bernoulli", "binomial"):
        return np.abs(y * f) + (n if lik == "binomial" else 1.0) * orc.softplus(f)
    if lik == "poisson_exp":
        return np.abs(y * f) + np.exp(f)
    g = orc.softplus(f)
    return np.abs(y * np.log(g)) + g


def bound(f, S):
    """The per-element bound on |got - ref|"""
    return c_of(f) * EPS * np.asarray(S, dtype=float) + ABS_FLOOR


def worst(got, want, bnd):
    """(index of the worst element, its ratio to the bound); a non-finite value counts as infinitely far off"""
    got, want, bnd = np.broadcast_arrays(np.asarray(got, float), np.asarray(want, float), np.asarray(bnd, float))
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(got == want, 0.0, np.where(np.isfinite(got), np.abs(got - want) / bnd, np.inf))
    i = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return i, float(ratio[i])


# ---- float32 restatements of the device formulas (numpy, correctly rounded exp / log) ---------------------------------
_f32 = np.float32


def _exp32(x, flush):
    with np.errstate(under="ignore", over="ignore"):
        t = np.exp(x.astype(_f32)).astype(_f32)
    return np.where(t < _f32(2.0 ** -126), _f32(0), t).astype(_f32) if flush else t


def _q32(t):
    """(log1p(t), log1p(t) / t) for 0 <= t <= 1 as rr_log1p01 forms them: log(u) t / (u - 1) with u = fl(1 + t); t and 1
    where u == 1"""
    u = (_f32(1) + t).astype(_f32)
    dd = (u - _f32(1)).astype(_f32)
    one = dd == 0
    dds = np.where(one, _f32(1), dd).astype(_f32)
    lu = np.log(u).astype(_f32)
    l1p = np.where(one, t, (lu * (t / dds).astype(_f32)).astype(_f32)).astype(_f32)
    q = np.where(one, _f32(1), (lu / dds).astype(_f32)).astype(_f32)
    return l1p, q


def emulate_f32(lik, y, f, n=1.0, fixed=True, flush=False):
    """(df, ll) of the float32 device formulas (rr_lik_elem, rr_elbo.hip) in numpy float32.  fixed=False: the Poisson-softplus
    element as it was before its rewrite (a clamp of g at 1e-37 and a division by it).  flush: exp results below the normal
    range become 0, as the hardware's exp2 returns them."""
    y, f, n = [np.asarray(a, dtype=_f32) for a in np.broadcast_arrays(np.asarray(y, _f32), np.asarray(f, _f32), np.asarray(n, _f32))]
    with np.errstate(all="ignore"):
        if lik == "poisson_exp":
            g = _exp32(f, flush)
            return (y - g).astype(_f32), ((y * f).astype(_f32) - g).astype(_f32)
        t = _exp32(-np.abs(f), flush)
        l1p, q = _q32(t)
        opt = (_f32(1) + t).astype(_f32)
        expit = np.where(f >= 0, _f32(1) / opt, t / opt).astype(_f32)
        sp = (np.maximum(f, _f32(0)) + l1p).astype(_f32)
        if lik in ("bernoulli", "binomial"):
            nn = n if lik == "binomial" else np.ones_like(f)
            return (y - (nn * expit).astype(_f32)).astype(_f32), ((y * f).astype(_f32) - (nn * sp).astype(_f32)).astype(_f32)
        if not fixed:
            g = np.maximum(sp, _f32(1e-37)).astype(_f32)
            df = (expit * ((y / g).astype(_f32) - _f32(1)).astype(_f32)).astype(_f32)
            return df, ((y * np.log(g).astype(_f32)).astype(_f32) - g).astype(_f32)
        # g = max(f, 0) + t q with q = log1p(t) / t in [log 2, 1].  f >= 0: g >= log 2, the plain formulas.  f < 0: g = t q, so
        # that expit(f) y / g = y / ((1 + t) q) and log g = f + log q: no division by g, nothing to clamp
        neg = f < 0
        g = (np.maximum(f, _f32(0)) + (t * q).astype(_f32)).astype(_f32)
        gp = np.where(neg, _f32(1), g).astype(_f32)
        df_p = (expit * ((y / gp).astype(_f32) - _f32(1)).astype(_f32)).astype(_f32)
        ll_p = ((y * np.log(gp).astype(_f32)).astype(_f32) - g).astype(_f32)
        df_n = ((y / (opt * q).astype(_f32)).astype(_f32) - expit).astype(_f32)
        ll_n = ((y * (f + np.log(q).astype(_f32)).astype(_f32)).astype(_f32) - g).astype(_f32)
        return np.where(neg, df_n, df_p).astype(_f32), np.where(neg, ll_n, ll_p).astype(_f32)
