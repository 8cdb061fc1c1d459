// Predictive statistics of the generalised linear model on the device (glm.py:324-570 of the reference): from the latent
// samples FSt[r][s] = Phi_r . w_s that rr_featmat_project's GEMM leaves in HBM (float32, rows x ld, S valid columns) to the
// two or three numbers per query row a caller wants back --
//   moments   mean and variance over the samples of the likelihood's Ey(f)                         glm.py:351-393
//   logpdf    mean / min / max over the samples of loglike(y_r, f)                                 glm.py:395-444
//   cdf       mean / min / max over the samples of cdf(q, f)                                       glm.py:446-495
//   interval  the two quantiles of the sample-averaged CDF, by the bisection of glm._bisect_quantile glm.py:497-570
// One wave per query row, 4 rows per 256-thread workgroup; the lanes stride over the S columns (coalesced), accumulate in
// float64 and are reduced with an xor butterfly, which leaves every lane with the SAME sum: the bisection's decisions are
// wave-uniform and nothing is atomic, so the results are the same bits every run.  Everything per row that does not depend
// on the sample (the lgamma terms of the count log-likelihoods, 1 / sqrt(2 var)) is formed once per row.
//
// The likelihood formulas are revrand_amd/likelihoods.py's, in float64, with the link value (p = expit(f), mu = exp(f) or
// softplus(f)) formed first as there.  The count CDFs are sums of the probability mass function that START AT THE ARGUMENT
// AND WALK AWAY FROM THE MODE (terms decrease from the first one on, so the sum stops after ~9 standard deviations):
//   Poisson   P(X <= k) = sum_{j <= k} pmf(j)      (k <  mu: downwards from k)
//                       = 1 - sum_{j > k} pmf(j)   (k >= mu: upwards from k + 1)   = Q(k + 1, mu)
//   binomial  the same two sums on either side of the mode (n + 1) p                = I_{1-p}(n - k, k + 1)
// The first term comes from Loader's saddle-point form of the mass function (C. Loader, "Fast and accurate computation of
// binomial probabilities", 2000): exp(-stirlerr(k) - bd0(k, mu)) / sqrt(2 pi k), in which neither exp(-mu) nor mu^k is ever
// formed -- relative error ~1e-15 for mu from 1e-8 to 1e6 and beyond, where exp(k log mu - mu - lgamma(k + 1)) loses
// mu * 1e-16.
#include "rr_internal.h"

#include <cmath>

namespace {

constexpr double kLn2Pi = 1.837877066409345483560659472811;      // log(2 pi)
constexpr double kHalfLn2Pi = 0.918938533204672741780329736406;  // log(2 pi) / 2
constexpr double kTwoPi = 6.283185307179586476925286766559;
constexpr int kMaxTerms = 65536;   // of a mass-function sum: ~9 sqrt(mu) terms are needed next to the mode (mu up to 5e7)
constexpr int kRegCols = 4;        // link values a lane keeps in registers: S <= 64 * kRegCols

__device__ __forceinline__ double pd_expit(double f) {
    if (f < 0.0) {
        const double t = exp(f);
        return t / (1.0 + t);
    }
    return 1.0 / (1.0 + exp(-f));
}

__device__ __forceinline__ double pd_softplus(double f) { return fmax(f, 0.0) + log1p(exp(-fabs(f))); }

// lgamma(n + 1) - ((n + 1/2) log n - n + log(2 pi) / 2) for n > 0: Stirling's series (the first neglected term is 1e-16 at 16)
__device__ double pd_stirlerr(double n) {
    if (n < 16.0) return lgamma(n + 1.0) - ((n + 0.5) * log(n) - n + kHalfLn2Pi);
    const double i2 = 1.0 / (n * n);
    return (1.0 / 12.0 - (1.0 / 360.0 - (1.0 / 1260.0 - (1.0 / 1680.0 - (1.0 / 1188.0) * i2) * i2) * i2) * i2) / n;
}

// x log(x / np) + np - x without the cancellation for x close to np
__device__ double pd_bd0(double x, double np) {
    if (fabs(x - np) < 0.1 * (x + np)) {
        double v = (x - np) / (x + np);
        double s = (x - np) * v;
        double ej = 2.0 * x * v;
        v = v * v;
        for (int j = 1; j < 1000; ++j) {
            ej *= v;
            const double s1 = s + ej / (double)(2 * j + 1);
            if (s1 == s) return s1;
            s = s1;
        }
        return s;
    }
    return x * log(x / np) + np - x;
}

// Poisson mass at an integer x >= 0
__device__ double pd_pois_pmf(double x, double mu) {
    if (mu == 0.0) return x == 0.0 ? 1.0 : 0.0;
    if (x == 0.0) return exp(-mu);
    return exp(-pd_stirlerr(x) - pd_bd0(x, mu)) / sqrt(kTwoPi * x);
}

// poisson.cdf(y, mu) = Q(floor(y) + 1, mu)
__device__ double pd_pois_cdf(double y, double mu) {
    if (y < 0.0) return 0.0;
    double x = floor(y);
    if (x < mu) {   // below the mode: pmf(x) + pmf(x - 1) + ...
        double t = pd_pois_pmf(x, mu), s = t;
        const double imu = 1.0 / mu;
        for (int it = 0; it < kMaxTerms && x >= 1.0; ++it) {
            t *= x * imu;
            x -= 1.0;
            s += t;
            if (t <= s * 1e-17) break;
        }
        return fmin(s, 1.0);
    }
    x += 1.0;       // at or above it: 1 - (pmf(x + 1) + pmf(x + 2) + ...)
    double t = pd_pois_pmf(x, mu), s = t;
    for (int it = 0; it < kMaxTerms; ++it) {
        if (t <= s * 1e-17) break;
        x += 1.0;
        t *= mu / x;
        s += t;
    }
    return fmax(1.0 - s, 0.0);
}

// binomial mass at an integer 0 <= x <= n, q = 1 - p
__device__ double pd_binom_pmf(double x, double n, double p, double q) {
    if (p == 0.0) return x == 0.0 ? 1.0 : 0.0;
    if (q == 0.0) return x == n ? 1.0 : 0.0;
    if (x == 0.0) {
        if (n == 0.0) return 1.0;
        return exp(p < 0.1 ? -pd_bd0(n, n * q) - n * p : n * log(q));
    }
    if (x == n) return exp(q < 0.1 ? -pd_bd0(n, n * p) - n * q : n * log(p));
    if (x < 0.0 || x > n) return 0.0;
    const double lc = pd_stirlerr(n) - pd_stirlerr(x) - pd_stirlerr(n - x) - pd_bd0(x, n * p) - pd_bd0(n - x, n * q);
    const double lf = kLn2Pi + log(x) + log1p(-x / n);
    return exp(lc - 0.5 * lf);
}

// binom.cdf(y, n, p) = I_{1-p}(n - k, k + 1), k = floor(y); q = 1 - p is formed from p as the host forms it
__device__ double pd_binom_cdf(double y, double n, double p) {
    if (y < 0.0) return 0.0;
    double x = floor(y);
    if (x >= n) return 1.0;
    const double q = 1.0 - p;
    if (q == 0.0) return 0.0;
    if (p == 0.0) return 1.0;
    if ((n - x) * p < (x + 1.0) * q) {   // pmf(x + 1) < pmf(x): at or above the mode, sum the upper tail
        x += 1.0;
        double t = pd_binom_pmf(x, n, p, q), s = t;
        const double r = p / q;
        for (int it = 0; it < kMaxTerms && x < n; ++it) {
            if (t <= s * 1e-17) break;
            t *= (n - x) / (x + 1.0) * r;
            x += 1.0;
            s += t;
        }
        return fmax(1.0 - s, 0.0);
    }
    double t = pd_binom_pmf(x, n, p, q), s = t;
    const double r = q / p;
    for (int it = 0; it < kMaxTerms && x >= 1.0; ++it) {
        if (t <= s * 1e-17) break;
        t *= x / (n - x + 1.0) * r;
        x -= 1.0;
        s += t;
    }
    return fmin(s, 1.0);
}

// ---- the five likelihoods: link value, Ey, cdf, loglike ---------------------------------------------------------
// link: what the sample's f enters Ey and cdf through -- p = expit(f) (Bernoulli, binomial), f (Gaussian), mu (Poisson)
template <int LIK>
__device__ __forceinline__ double pd_link(double f) {
    if constexpr (LIK == RR_LIK_BERNOULLI || LIK == RR_LIK_BINOMIAL) return pd_expit(f);
    else if constexpr (LIK == RR_LIK_POISSON_EXP) return exp(f);
    else if constexpr (LIK == RR_LIK_POISSON_SOFTPLUS) return pd_softplus(f);
    else return f;
}

template <int LIK>
__device__ __forceinline__ double pd_ey(double link, double n) {
    if constexpr (LIK == RR_LIK_BINOMIAL) return link * n;
    else return link;
}

// isd2 = 1 / sqrt(2 var) (Gaussian)
template <int LIK>
__device__ __forceinline__ double pd_cdf(double y, double link, double n, double isd2) {
    if constexpr (LIK == RR_LIK_BERNOULLI) return y < 0.0 ? 0.0 : (y < 1.0 ? 1.0 - link : 1.0);
    else if constexpr (LIK == RR_LIK_BINOMIAL) return pd_binom_cdf(y, n, link);
    else if constexpr (LIK == RR_LIK_GAUSSIAN) return 0.5 * erfc(-(y - link) * isd2);
    else return pd_pois_cdf(y, link);
}

// the part of loglike that depends on the row only: log C(n, y) (-inf outside the support), log(2 pi var), gammaln(y + 1)
template <int LIK>
__device__ __forceinline__ double pd_rowconst(double y, double n, double var) {
    if constexpr (LIK == RR_LIK_BINOMIAL) {
        if (!(y >= 0.0 && y <= n && y == floor(y))) return -INFINITY;
        return lgamma(n + 1.0) - (lgamma(y + 1.0) + lgamma(n - y + 1.0));
    } else if constexpr (LIK == RR_LIK_GAUSSIAN) {
        return log(kTwoPi * var);
    } else if constexpr (LIK == RR_LIK_POISSON_EXP || LIK == RR_LIK_POISSON_SOFTPLUS) {
        return lgamma(y + 1.0);
    } else {
        return 0.0;
    }
}

template <int LIK>
__device__ __forceinline__ double pd_loglike(double y, double f, double n, double var, double c0) {
    if constexpr (LIK == RR_LIK_BERNOULLI) {
        return y * f - pd_softplus(f);
    } else if constexpr (LIK == RR_LIK_BINOMIAL) {   // binom.logpmf: combiln + xlogy(k, p) + xlog1py(n - k, -p)
        if (c0 == -INFINITY) return c0;
        const double p = pd_expit(f), m = n - y;
        return c0 + (y == 0.0 ? 0.0 : y * log(p)) + (m == 0.0 ? 0.0 : m * log1p(-p));
    } else if constexpr (LIK == RR_LIK_GAUSSIAN) {
        const double e = y - f;
        return -0.5 * (c0 + e * e / var);
    } else if constexpr (LIK == RR_LIK_POISSON_EXP) {
        return y * f - exp(f) - c0;
    } else {
        const double g = pd_softplus(f);
        return y * log(g) - g - c0;
    }
}

__device__ __forceinline__ double pd_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ double pd_wave_min(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ __forceinline__ double pd_wave_max(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
    return v;
}

// mean over the row's samples of cdf(q, .): the lane's link values from registers (REG) or formed again from the row
template <int LIK, bool REG>
__device__ __forceinline__ double pd_mean_cdf(double q, const double (&v)[kRegCols], const float *__restrict__ row, int S,
                                              int lane, double n, double isd2) {
    double acc = 0.0;
    if constexpr (REG) {
#pragma unroll
        for (int i = 0; i < kRegCols; ++i)
            if (lane + 64 * i < S) acc += pd_cdf<LIK>(q, v[i], n, isd2);
    } else {
        for (int col = lane; col < S; col += 64) acc += pd_cdf<LIK>(q, pd_link<LIK>((double)row[col]), n, isd2);
    }
    return pd_wave_sum(acc) / (double)S;
}

// The CDF of a count likelihood depends on floor(q) only, and a bisection spends most of its 100 halvings inside one unit
// interval: the last two evaluated steps are kept (step_cache; wave-uniform values, so the reuse returns the very bits an
// evaluation would).
struct StepCache {
    double k0, m0, k1, m1;   // (floor(q), mean) of the last and the last-but-one evaluated step
};

template <int LIK, bool REG>
__device__ __forceinline__ double pd_mean_cdf_cached(double q, StepCache &sc, int step_cache, const double (&v)[kRegCols],
                                                     const float *__restrict__ row, int S, int lane, double n, double isd2) {
    if constexpr (LIK == RR_LIK_GAUSSIAN) {
        return pd_mean_cdf<LIK, REG>(q, v, row, S, lane, n, isd2);
    } else {
        if (!step_cache) return pd_mean_cdf<LIK, REG>(q, v, row, S, lane, n, isd2);
        if (q < 0.0) return 0.0;   // (every sample's CDF is exactly 0 there)
        const double kq = floor(q);
        if (kq == sc.k0) return sc.m0;
        if (kq == sc.k1) return sc.m1;
        const double m = pd_mean_cdf<LIK, REG>(q, v, row, S, lane, n, isd2);
        sc.k1 = sc.k0;
        sc.m1 = sc.m0;
        sc.k0 = kq;
        sc.m0 = m;
        return m;
    }
}

// glm._bisect_quantile for one row: bracket [-reach, reach], 100 halvings, NaN when the bracket does not straddle p
template <int LIK, bool REG>
__device__ __forceinline__ double pd_bisect(double p, double reach, StepCache &sc, int step_cache, const double (&v)[kRegCols],
                                            const float *__restrict__ row, int S, int lane, double n, double isd2) {
    double lo = -reach, hi = reach;
    const double clo = pd_mean_cdf_cached<LIK, REG>(lo, sc, step_cache, v, row, S, lane, n, isd2);
    const double chi = pd_mean_cdf_cached<LIK, REG>(hi, sc, step_cache, v, row, S, lane, n, isd2);
    const bool inside = (clo <= p) && (chi >= p);
    for (int it = 0; it < 100; ++it) {
        const double mid = 0.5 * (lo + hi);
        const bool below = pd_mean_cdf_cached<LIK, REG>(mid, sc, step_cache, v, row, S, lane, n, isd2) < p;
        lo = below ? mid : lo;
        hi = below ? hi : mid;
    }
    return inside ? 0.5 * (lo + hi) : NAN;
}

// what: RR_PRED_*.  out (rows, 2): moments (Ey, Vy), interval (lower, upper); (rows, 3): logpdf / cdf (mean, min, max).
// REG (moments, interval; S <= 64 * kRegCols): the lane's per-sample values stay in registers between the passes; otherwise
// the second pass / every CDF evaluation reads the row again (from L2) and forms them again.
template <int LIK, int WHAT, bool REG>
__global__ void __launch_bounds__(256)
rr_predictive_kernel(const float *__restrict__ FSt, int64_t rows, int S, int64_t ld, double var,
                     const double *__restrict__ rowarg, const double *__restrict__ yrow, double q, double p_lo, double p_hi,
                     int step_cache, double *__restrict__ out) {
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    RR_DEV_ASSERT(S >= 1 && (int64_t)S <= ld && (!REG || S <= 64 * kRegCols));
    RR_DEV_ASSERT(LIK != RR_LIK_BINOMIAL || rowarg != nullptr);
    RR_DEV_ASSERT(WHAT != RR_PRED_LOGPDF || yrow != nullptr);
    const float *__restrict__ row = FSt + r * ld;
    double n = 0.0;
    if constexpr (LIK == RR_LIK_BINOMIAL) n = rowarg[r];
    const double isd2 = LIK == RR_LIK_GAUSSIAN ? 1.0 / sqrt(2.0 * var) : 0.0;
    double v[kRegCols] = {0.0, 0.0, 0.0, 0.0};

    if constexpr (WHAT == RR_PRED_MOMENTS) {
        double acc = 0.0;
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < kRegCols; ++i)
                if (lane + 64 * i < S) {
                    v[i] = pd_ey<LIK>(pd_link<LIK>((double)row[lane + 64 * i]), n);
                    acc += v[i];
                }
        } else {
            for (int col = lane; col < S; col += 64) acc += pd_ey<LIK>(pd_link<LIK>((double)row[col]), n);
        }
        const double mean = pd_wave_sum(acc) / (double)S;
        double dev = 0.0;   // the mean of the squared deviations from that mean: a second pass, as the host makes it
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < kRegCols; ++i)
                if (lane + 64 * i < S) dev += (v[i] - mean) * (v[i] - mean);
        } else {
            for (int col = lane; col < S; col += 64) {
                const double e = pd_ey<LIK>(pd_link<LIK>((double)row[col]), n) - mean;
                dev += e * e;
            }
        }
        dev = pd_wave_sum(dev) / (double)S;
        if (lane == 0) {
            out[r * 2] = mean;
            out[r * 2 + 1] = dev;
        }
    } else if constexpr (WHAT == RR_PRED_LOGPDF || WHAT == RR_PRED_CDF) {
        const double y = WHAT == RR_PRED_LOGPDF ? yrow[r] : q;
        const double c0 = WHAT == RR_PRED_LOGPDF ? pd_rowconst<LIK>(y, n, var) : 0.0;
        double acc = 0.0, mn = INFINITY, mx = -INFINITY;
        for (int col = lane; col < S; col += 64) {
            const double f = (double)row[col];
            const double t = WHAT == RR_PRED_LOGPDF ? pd_loglike<LIK>(y, f, n, var, c0) : pd_cdf<LIK>(y, pd_link<LIK>(f), n, isd2);
            acc += t;
            mn = fmin(mn, t);
            mx = fmax(mx, t);
        }
        acc = pd_wave_sum(acc) / (double)S;
        mn = pd_wave_min(mn);
        mx = pd_wave_max(mx);
        if (lane == 0) {
            out[r * 3] = acc;
            out[r * 3 + 1] = mn;
            out[r * 3 + 2] = mx;
        }
    } else {   // RR_PRED_INTERVAL
        double acc = 0.0;
        if constexpr (REG) {
#pragma unroll
            for (int i = 0; i < kRegCols; ++i)
                if (lane + 64 * i < S) {
                    v[i] = pd_link<LIK>((double)row[lane + 64 * i]);
                    acc += pd_ey<LIK>(v[i], n);
                }
        } else {
            for (int col = lane; col < S; col += 64) acc += pd_ey<LIK>(pd_link<LIK>((double)row[col]), n);
        }
        const double centre = pd_wave_sum(acc) / (double)S;
        const double reach = 1000.0 * fmax(centre, 1.0);
        StepCache sc;
        sc.k0 = sc.k1 = -1.0;   // (floor of a non-negative argument is never -1)
        sc.m0 = sc.m1 = 0.0;
        const double ql = pd_bisect<LIK, REG>(p_lo, reach, sc, step_cache, v, row, S, lane, n, isd2);
        const double qu = pd_bisect<LIK, REG>(p_hi, reach, sc, step_cache, v, row, S, lane, n, isd2);
        if (lane == 0) {
            out[r * 2] = ql;
            out[r * 2 + 1] = qu;
        }
    }
}

// elementwise loglike / Ey / cdf on float64 arrays, through the device functions above (rr_lik_eval)
template <int LIK>
__global__ void __launch_bounds__(256)
rr_lik_eval_kernel(int what, double var, const double *__restrict__ y, const double *__restrict__ f,
                   const double *__restrict__ rowarg, int64_t cnt, double *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= cnt) return;
    RR_DEV_ASSERT(LIK != RR_LIK_BINOMIAL || rowarg != nullptr);
    RR_DEV_ASSERT(what == RR_EVAL_EY || y != nullptr);
    double n = 0.0;
    if constexpr (LIK == RR_LIK_BINOMIAL) n = rowarg[i];
    const double fi = f[i];
    if (what == RR_EVAL_EY) out[i] = pd_ey<LIK>(pd_link<LIK>(fi), n);
    else if (what == RR_EVAL_LOGLIKE) out[i] = pd_loglike<LIK>(y[i], fi, n, var, pd_rowconst<LIK>(y[i], n, var));
    else out[i] = pd_cdf<LIK>(y[i], pd_link<LIK>(fi), n, LIK == RR_LIK_GAUSSIAN ? 1.0 / sqrt(2.0 * var) : 0.0);
}

template <int LIK, int WHAT>
void launch_what(rr_ctx *c, bool reg, const float *FSt, int64_t rows, int S, int64_t ld, double var, const double *drowarg,
                 const double *dy, double q, double p_lo, double p_hi, int step_cache, double *dout) {
    const dim3 grid((unsigned)((rows + 3) / 4));
    if constexpr (WHAT == RR_PRED_MOMENTS || WHAT == RR_PRED_INTERVAL) {   // (the one-pass statistics keep nothing)
        if (reg) {
            hipLaunchKernelGGL((rr_predictive_kernel<LIK, WHAT, true>), grid, dim3(256), 0, c->stream, FSt, rows, S, ld, var,
                               drowarg, dy, q, p_lo, p_hi, step_cache, dout);
            return;
        }
    }
    hipLaunchKernelGGL((rr_predictive_kernel<LIK, WHAT, false>), grid, dim3(256), 0, c->stream, FSt, rows, S, ld, var, drowarg,
                       dy, q, p_lo, p_hi, step_cache, dout);
}

template <int LIK>
void launch_lik(rr_ctx *c, int what, const float *FSt, int64_t rows, int S, int64_t ld, double var, const double *drowarg,
                const double *dy, double q, double p_lo, double p_hi, double *dout) {
    // RR_PRED_NO_REG=1 / RR_PRED_NO_STEP_CACHE=1: measurement switches (tools/glm_predict_bench.py)
    static const bool no_reg = getenv("RR_PRED_NO_REG") != nullptr;
    static const bool no_cache = getenv("RR_PRED_NO_STEP_CACHE") != nullptr;
    const bool reg = S <= 64 * kRegCols && !no_reg;
    const int sc = no_cache ? 0 : 1;
    switch (what) {
    case RR_PRED_MOMENTS: launch_what<LIK, RR_PRED_MOMENTS>(c, reg, FSt, rows, S, ld, var, drowarg, dy, q, p_lo, p_hi, sc, dout); break;
    case RR_PRED_LOGPDF: launch_what<LIK, RR_PRED_LOGPDF>(c, false, FSt, rows, S, ld, var, drowarg, dy, q, p_lo, p_hi, sc, dout); break;
    case RR_PRED_CDF: launch_what<LIK, RR_PRED_CDF>(c, false, FSt, rows, S, ld, var, drowarg, dy, q, p_lo, p_hi, sc, dout); break;
    default: launch_what<LIK, RR_PRED_INTERVAL>(c, reg, FSt, rows, S, ld, var, drowarg, dy, q, p_lo, p_hi, sc, dout); break;
    }
}

}  // namespace

int rr_predictive_out_cols(int what) { return (what == RR_PRED_LOGPDF || what == RR_PRED_CDF) ? 3 : 2; }

int rr_launch_predictive(rr_ctx *c, const float *FSt, int64_t rows, int S, int64_t ld, int what, int lik, double lik_param,
                         const double *drowarg, const double *dy, double q, double p_lo, double p_hi, double *dout) {
    RR_REQUIRE(c != nullptr && FSt != nullptr && dout != nullptr && rows >= 1 && S >= 1 && (int64_t)S <= ld,
               "predictive kernel: bad extents");
    RR_REQUIRE(what >= RR_PRED_MOMENTS && what <= RR_PRED_INTERVAL, "predictive kernel: unknown statistic %d", what);
    switch (lik) {
    case RR_LIK_BERNOULLI: launch_lik<RR_LIK_BERNOULLI>(c, what, FSt, rows, S, ld, lik_param, drowarg, dy, q, p_lo, p_hi, dout); break;
    case RR_LIK_BINOMIAL: launch_lik<RR_LIK_BINOMIAL>(c, what, FSt, rows, S, ld, lik_param, drowarg, dy, q, p_lo, p_hi, dout); break;
    case RR_LIK_GAUSSIAN: launch_lik<RR_LIK_GAUSSIAN>(c, what, FSt, rows, S, ld, lik_param, drowarg, dy, q, p_lo, p_hi, dout); break;
    case RR_LIK_POISSON_EXP: launch_lik<RR_LIK_POISSON_EXP>(c, what, FSt, rows, S, ld, lik_param, drowarg, dy, q, p_lo, p_hi, dout); break;
    case RR_LIK_POISSON_SOFTPLUS: launch_lik<RR_LIK_POISSON_SOFTPLUS>(c, what, FSt, rows, S, ld, lik_param, drowarg, dy, q, p_lo, p_hi, dout); break;
    default: RR_REQUIRE(false, "predictive kernel: unknown likelihood %d", lik);
    }
    RR_CHECK_HIP(hipGetLastError());
    return RR_OK;
}

// what the predictive entry points share: likelihood id, its parameter and its per-row argument
int rr_predictive_check_lik(const char *who, int lik, double lik_param, const void *rowarg) {
    RR_REQUIRE(lik >= RR_LIK_BERNOULLI && lik <= RR_LIK_POISSON_SOFTPLUS, "%s: unknown likelihood %d", who, lik);
    RR_REQUIRE(lik != RR_LIK_BINOMIAL || rowarg != nullptr, "%s: the binomial likelihood needs its per-row n", who);
    RR_REQUIRE(lik != RR_LIK_GAUSSIAN || lik_param > 0.0, "%s: the Gaussian likelihood needs a positive variance", who);
    return RR_OK;
}

extern "C" {

int rr_lik_eval(rr_ctx *ctx, int what, int lik, double lik_param, const double *y, const double *f, const double *rowarg,
                int64_t n, double *out) {
    RR_REQUIRE(ctx != nullptr && n >= 0, "rr_lik_eval: bad argument");
    RR_REQUIRE(what >= RR_EVAL_LOGLIKE && what <= RR_EVAL_CDF, "rr_lik_eval: unknown function %d", what);
    int rc = rr_predictive_check_lik("rr_lik_eval", lik, lik_param, rowarg);
    if (rc != RR_OK) return rc;
    if (n == 0) return RR_OK;
    RR_REQUIRE(f != nullptr && out != nullptr && (what == RR_EVAL_EY || y != nullptr), "rr_lik_eval: null array");
    RR_CHECK_HIP(hipSetDevice(ctx->device));
    // one allocation: [y | f | rowarg | out]
    double *d = nullptr;
    RR_CHECK_HIP(hipMalloc((void **)&d, (size_t)n * 4 * sizeof(double)));
    double *dy = d, *df = d + n, *dn = d + 2 * n, *dout = d + 3 * n;
    const size_t bytes = (size_t)n * sizeof(double);
    hipError_t e = hipMemcpyAsync(df, f, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && y) e = hipMemcpyAsync(dy, y, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess && lik == RR_LIK_BINOMIAL) e = hipMemcpyAsync(dn, rowarg, bytes, hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        const dim3 grid((unsigned)((n + 255) / 256));
        const double *cy = y ? dy : nullptr, *cn = lik == RR_LIK_BINOMIAL ? dn : nullptr;
        switch (lik) {
        case RR_LIK_BERNOULLI: hipLaunchKernelGGL(rr_lik_eval_kernel<RR_LIK_BERNOULLI>, grid, dim3(256), 0, ctx->stream, what, lik_param, cy, (const double *)df, cn, n, dout); break;
        case RR_LIK_BINOMIAL: hipLaunchKernelGGL(rr_lik_eval_kernel<RR_LIK_BINOMIAL>, grid, dim3(256), 0, ctx->stream, what, lik_param, cy, (const double *)df, cn, n, dout); break;
        case RR_LIK_GAUSSIAN: hipLaunchKernelGGL(rr_lik_eval_kernel<RR_LIK_GAUSSIAN>, grid, dim3(256), 0, ctx->stream, what, lik_param, cy, (const double *)df, cn, n, dout); break;
        case RR_LIK_POISSON_EXP: hipLaunchKernelGGL(rr_lik_eval_kernel<RR_LIK_POISSON_EXP>, grid, dim3(256), 0, ctx->stream, what, lik_param, cy, (const double *)df, cn, n, dout); break;
        default: hipLaunchKernelGGL(rr_lik_eval_kernel<RR_LIK_POISSON_SOFTPLUS>, grid, dim3(256), 0, ctx->stream, what, lik_param, cy, (const double *)df, cn, n, dout); break;
        }
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, dout, bytes, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d);
    if (e != hipSuccess) {
        rr_set_error("rr_lik_eval failed: %s", hipGetErrorString(e));
        return RR_ERR_HIP;
    }
    return RR_OK;
}

}  // extern "C"
