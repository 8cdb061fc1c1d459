// The small-minibatch regime of GeneralizedLinearModel.fit (rr_svi.hip) for WIDE bases: the reference's report runs batch 10,
// K = 10, 50 samples at nbases 256 ... 8192, F = 512 ... 16384, where (m, C) of one component alone no longer fits a CU's LDS.
//
// rr_svi.hip keeps K workgroups inside one kernel and orders them with device-scope barriers; that needs co-residency and
// does not grow.  Here NO workgroup ever waits for another: a step is a fixed chain of FOUR kernels on the context's stream
// and the kernel boundary is the only ordering between workgroups; `steps` chains are queued per library call.  The basis is
// cut into ITEMS (rr_glm_sviw_plan: a run of frequencies of one random Fourier child with BOTH their columns, or one whole
// linear child; rr_glm_sviwgm_plan: also a run of frequencies of one spectral-mixture component with all FOUR their columns),
// and every sum over the basis is "each (item, component) workgroup stores its partial, a later kernel adds
// the partials in item order": no floating-point atomics, the same bits every run and for every cut of a fit into calls.
//
//   A  grid (items, K)   mk, sk of the item's columns; the minibatch rows gathered by index; Phi of the item (component 0's
//                        workgroup stores it for C); the draws of component k (the caller's or rr_svi_draw's); the item's partial
//                        of fs[k, l, r] = ws Phi^T; its partial of row k of the mixture's cross terms q and of sum (m^2 + C)
//   B  grid (blocks, K)  fs = the partials in item order; dfs and the log-likelihood sums per block (rr_svi_lik's formulas);
//                        block 0 of component k: q[k][.] and sum (m^2 + C) per child in item order
//   C  grid (items, K)   log N, log z, alpha from q; D_r = sum_l dfs, Q = dfs^T e of the item; Edm, EdC; the gradient of the
//                        item's 2 w coordinates of component k, log trick, |g|^2 partial, bounds, updater, clip; the item's
//                        partial of the child's length-scale contractions
//   D  one workgroup     the partials of C in item order; the shared coordinates (regularisers, Gaussian variance, length
//                        scales); the step's -ELBO and |g|
//
// x = from_log(z) lives in HBM twice, by step parity: a step reads x[t & 1] and writes x[(t + 1) & 1] (C its own coordinates,
// D the shared ones), so no kernel reads what a neighbour of the same launch writes.  rr_glm_sviw_starts runs A, B and D
// (objective only) per candidate, the candidate's x in place of x[t & 1].
// Everything is float64 (the draws are float32 values); no lgamma, no pow: dlconst and Adam's bias come from the host.
#include "rr_internal.h"
#include "rr_svi_common.h"

#include <algorithm>
#include <cstdlib>

#define SW_MAXCHILD 16
#define SW_MAXK 32
#define SW_MAXL 128
#define SW_MAXM 64
#define SW_MAXF 32768
#define SW_MAXD 128
#define SW_THREADS 512
#define SW_WAVES (SW_THREADS / 64)
#define SW_ITEM_DEFAULT 64                   // frequencies per item at most (LDS permitting)
#define SW_ITEM_GM_DEFAULT 32                // ... of a spectral-mixture component: 4 columns each, the same 128 columns per item
#define SW_MAXLS (2 * SW_MAXD)               // slots of one child at most: a spectral-mixture component's [mean | length scales]
#define SW_LDS_BUDGET (156 * 1024)           // what an item may take of a CU's 160 KiB
#define SW_SCRATCH_MAX ((int64_t)2 << 30)    // the partials of fs (items K L M doubles) stay below this
#define SW_LAUNCHES_PER_STEP 4
#define SW_LAUNCHES_PER_START 3

namespace {

struct SwChild {
    int kind, col0, width, d, n, n_ls, ls0, onescol, x_f64, item0, nitems;
    const void *X;
    int64_t ldx;
    const double *W;   // RFF: raw (d, n) row-major on the device; GM: the dense equivalent V of the component's chain, likewise
};

struct SwItem {
    int child, j0, cnt;   // RFF: frequencies [j0, j0 + cnt) and both their columns (GM: all four); linear: columns [j0, j0 + cnt) = all
};

struct SwArgs {
    const SwChild *kid;
    const SwItem *items;
    int nitems, nkids, F, K, L, M, lik, n_lik, n_ls, ns, updater, y_f64, maxls, nbx, objective_only;
    int64_t np, N;
    const void *y, *rowarg;
    const double *lconst;
    double *z, *s1, *s2;
    const double *lower, *upper;
    const unsigned char *islog;
    const double *xin;   // x of this step (or the candidate)
    double *xout;        // x of the next step
    double *Phi, *fsp, *qp, *Rp, *dfs, *llp, *qf, *Rk, *n2p, *glsp;
    const float *E;      // this step's draws (K L, F) or null
    const int *idx;      // this step's rows (M)
    double *obj, *norm;  // where this step's (candidate's) record goes
    double up[4], bmag, b1t, b2t;
    uint64_t stepkey;
};

// sum over the block in a fixed order; every thread gets it (red: SW_WAVES doubles of LDS)
__device__ __forceinline__ double sw_block_sum(double v, ldsd *red) {
    const int tid = threadIdx.x;
    v = rr_svi_wave_sum(v);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = v;
    __syncthreads();
    double r = 0.0;
#pragma unroll
    for (int w = 0; w < SW_WAVES; ++w) r += red[w];
    return r;
}

// ---- what one item holds in LDS (doubles) in kernel A (stage 0) and kernel C (stage 1) -----------------------------------------
// A: the gathered rows, W / (2 pi l), Phi, mk, sk, the draws.  C: the same front part (W raw) plus dfs, Q, T, D_r, q, log z,
// alpha; a linear item of C keeps neither draws nor Q (each draw is used once there: read or made on the fly).
// rff: the column PAIRS [cos | sin] a frequency has -- 0 a linear item, 1 a random Fourier item, 2 a spectral-mixture item
// (cos+ | sin+ | cos- | sin-: w = 4 cnt), which adds mean / (2 pi) (d), the rows' b = x . mean / (2 pi) (M) and a second T.
struct SwLay {
    size_t Xb, Wl, mu, bb, Phi, mk, sk, Ef, dfs, Q, T, Dr, q, logz, alpha, red, total;
    int w, wp;
};

// GM: the instance with spectral-mixture items (rff may be 2).  The kernels are instantiated twice on it: a fit without such a
// child launches the <false> instances, whose code is what it was before these items existed.
template <bool GM>
static __host__ __device__ SwLay sw_layout(int rff, int cnt, int d, int K, int L, int M, int stage) {
    SwLay s;
    s.w = rff ? (GM ? 2 * rff * cnt : 2 * cnt) : cnt;
    s.wp = s.w | 1;   // odd row length of Phi: rows r, r + 1 of one column sit in different banks
    size_t o = 0;
    s.Xb = o; o += rff ? (size_t)M * d : 0;
    s.Wl = o; o += rff ? (size_t)d * cnt : 0;
    s.mu = o; o += (GM && rff == 2) ? d : 0;
    s.bb = o; o += (GM && rff == 2) ? M : 0;
    s.Phi = o; o += (size_t)M * s.wp;
    s.mk = o; o += s.w;
    s.sk = o; o += s.w;
    s.Ef = o; o += (rff || stage == 0) ? ((size_t)L * s.w + 1) / 2 : 0;
    s.dfs = o; o += stage ? (size_t)L * M : 0;
    s.Q = o; o += (stage && rff) ? (size_t)M * s.w : 0;
    s.T = o; o += (stage && rff) ? (size_t)(GM ? rff : 1) * M * cnt : 0;
    s.Dr = o; o += stage ? M : 0;
    s.q = o; o += stage ? (size_t)K * K : 0;
    s.logz = o; o += stage ? K : 0;
    s.alpha = o; o += stage ? K : 0;
    s.red = o; o += 8;
    s.total = o;
    return s;
}

static size_t sw_item_bytes(int rff, int cnt, int d, int K, int L, int M) {
    return 8 * std::max(sw_layout<true>(rff, cnt, d, K, L, M, 0).total, sw_layout<true>(rff, cnt, d, K, L, M, 1).total);
}

// the item's local column cc (< w) in the concatenation
template <bool GM>
__device__ __forceinline__ int sw_col(const SwChild &c, const SwItem &it, int cc) {
    if (c.kind == RR_SGD_CHILD_RFF) return c.col0 + (cc < it.cnt ? it.j0 + cc : c.n + it.j0 + (cc - it.cnt));
    if (GM && c.kind == RR_SGD_CHILD_GM) return c.col0 + (cc / it.cnt) * c.n + it.j0 + cc % it.cnt;   // block cc / cnt of cos+ | sin+ | cos- | sin-
    return c.col0 + it.j0 + cc;
}

template <bool GM>
__device__ __forceinline__ void sw_check_item(const SwArgs &a, const SwChild &c, const SwItem &it) {
    RR_DEV_ASSERT(GM || c.kind != RR_SGD_CHILD_GM);
    RR_DEV_ASSERT(it.child >= 0 && it.child < a.nkids && it.cnt >= 1 && it.j0 >= 0);
    RR_DEV_ASSERT(c.col0 >= 0 && c.col0 + c.width <= a.F);
    RR_DEV_ASSERT(c.kind == RR_SGD_CHILD_RFF ? (it.j0 + it.cnt <= c.n && c.width == 2 * c.n)
                  : c.kind == RR_SGD_CHILD_GM ? (it.j0 + it.cnt <= c.n && c.width == 4 * c.n && c.n_ls == 2 * c.d)
                                              : (it.j0 == 0 && it.cnt == c.width));
    RR_DEV_ASSERT(c.ls0 >= 0 && c.ls0 + c.n_ls <= a.n_ls && c.n_ls <= a.maxls);
}

// the item's draws of component k into LDS (L, w): the caller's or the device generator's -- the counter of rr_glm_draw_kernel
template <bool GM>
__device__ __forceinline__ void sw_draws(const SwArgs &a, const SwChild &c, const SwItem &it, int k, int w, ldsf *Ef) {
    const int tid = threadIdx.x, L = a.L, F = a.F;
    for (int o = tid; o < L * w; o += SW_THREADS) {
        const int l = o / w, col = sw_col<GM>(c, it, o % w);
        RR_DEV_ASSERT(col >= c.col0 && col < c.col0 + c.width);
        const uint64_t ctr = ((uint64_t)k * (uint64_t)L + (uint64_t)l) * (uint64_t)F + (uint64_t)col;
        Ef[o] = a.E ? a.E[ctr] : rr_svi_draw(a.stepkey, ctr);
    }
}

// the minibatch's rows of a random Fourier (or spectral-mixture) child's columns of X into LDS (M, d)
__device__ __forceinline__ void sw_gather(const SwArgs &a, const SwChild &c, ldsd *Xb) {
    for (int e = threadIdx.x; e < a.M * c.d; e += SW_THREADS) {
        const int r = e / c.d, i = e % c.d;
        const int64_t row = a.idx[r];
        RR_DEV_ASSERT(row >= 0 && row < a.N);
        Xb[e] = rr_svi_xval(c, row, i);
    }
}

// ---- A ------------------------------------------------------------------------------------------------------------------
template <bool GM>
__global__ void __launch_bounds__(SW_THREADS) rr_glm_sviw_a_kernel(const SwArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double sm[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, ii = blockIdx.x, k = blockIdx.y;
    const int K = a.K, F = a.F, L = a.L, M = a.M;
    RR_DEV_ASSERT(ii < a.nitems && k < K);
    const SwItem it = a.items[ii];
    const SwChild &c = a.kid[it.child];
    sw_check_item<GM>(a, c, it);
    const bool rff = c.kind == RR_SGD_CHILD_RFF, gm = GM && c.kind == RR_SGD_CHILD_GM;
    const SwLay s = sw_layout<GM>(gm ? 2 : rff, it.cnt, c.d, K, L, M, 0);
    const int w = s.w, wp = s.wp, cnt = it.cnt;
    ldsd *b = (ldsd *)sm;
    ldsd *Xb = b + s.Xb, *Wl = b + s.Wl, *Phi = b + s.Phi, *mk = b + s.mk, *sk = b + s.sk;
    ldsf *Ef = (ldsf *)(b + s.Ef);
    const int64_t fk = (int64_t)F * K;
    const double *xm = a.xin, *xC = a.xin + fk, *xs = a.xin + 2 * fk;
    for (int cc = tid; cc < w; cc += SW_THREADS) {
        const int col = sw_col<GM>(c, it, cc);
        mk[cc] = xm[(int64_t)col * K + k];
        sk[cc] = sqrt(xC[(int64_t)col * K + k]);
    }
    if (rff) {
        sw_gather(a, c, Xb);
        // W[i][j] / (2 pi l_i): phases in revolutions; the isotropic child has one length scale for every dimension
        for (int e = tid; e < c.d * cnt; e += SW_THREADS) {
            const int i = e / cnt, j = e % cnt;
            const double l = xs[a.nkids + a.n_lik + c.ls0 + (c.n_ls == 1 ? 0 : i)];
            Wl[e] = c.W[(size_t)i * c.n + it.j0 + j] * (0.15915494309189533576888 / l);
        }
    } else if (gm) {
        // a spectral-mixture component (basis_functions.py:1386-1562): slots [mean (d) | length scales (d)], both per input dimension
        ldsd *mu = b + s.mu;
        const double *sl = xs + a.nkids + a.n_lik + c.ls0;
        sw_gather(a, c, Xb);
        for (int e = tid; e < c.d * cnt; e += SW_THREADS) {
            const int i = e / cnt, j = e % cnt;
            Wl[e] = c.W[(size_t)i * c.n + it.j0 + j] * (0.15915494309189533576888 / sl[c.d + i]);
        }
        for (int i = tid; i < c.d; i += SW_THREADS) mu[i] = 0.15915494309189533576888 * sl[i];
    }
    sw_draws<GM>(a, c, it, k, w, Ef);
    __syncthreads();
    if (gm) {
        // b[r] = x_r . mean / (2 pi) ONCE per row, then cos(a + b) | sin(a + b) | cos(a - b) | sin(a - b), each / sqrt(2 n), with
        // a = x_r . V[:, j] / (2 pi l): the reference's column order (:1471-1473), rr_svi.hip's arithmetic (svi_features)
        ldsd *mu = b + s.mu, *bb = b + s.bb;
        for (int r = tid; r < M; r += SW_THREADS) {
            double t = 0.0;
            for (int i = 0; i < c.d; ++i) t = fma(Xb[r * c.d + i], mu[i], t);
            bb[r] = t;
        }
        __syncthreads();
        const double scale = 1.0 / sqrt(2.0 * (double)c.n);
        for (int e = tid; e < M * cnt; e += SW_THREADS) {
            const int r = e / cnt, j = e % cnt;
            double t = 0.0;
            for (int i = 0; i < c.d; ++i) t = fma(Xb[r * c.d + i], Wl[i * cnt + j], t);
            ldsd *ph = Phi + r * wp + j;
            const double br = bb[r];
#pragma unroll 1
            for (int sg = 0; sg < 2; ++sg, ph += 2 * cnt) {   // the + pair, then the - pair (one copy of the sincos code)
                double sn, cs;
                rr_sincos_rev_f64(sg ? t - br : t + br, sn, cs);
                ph[0] = cs * scale;
                ph[cnt] = sn * scale;
            }
        }
    } else if (rff) {
        const double scale = 1.0 / sqrt((double)c.n);
        for (int e = tid; e < M * cnt; e += SW_THREADS) {
            const int r = e / cnt, j = e % cnt;
            double t = 0.0;
            for (int i = 0; i < c.d; ++i) t = fma(Xb[r * c.d + i], Wl[i * cnt + j], t);
            double sn, cs;
            rr_sincos_rev_f64(t, sn, cs);
            Phi[r * wp + j] = cs * scale;
            Phi[r * wp + cnt + j] = sn * scale;
        }
    } else {
        RR_DEV_ASSERT(c.width == c.d + c.onescol);
        for (int e = tid; e < M * w; e += SW_THREADS) {
            const int r = e / w, j = e % w;
            const int64_t row = a.idx[r];
            RR_DEV_ASSERT(row >= 0 && row < a.N);
            Phi[r * wp + j] = (c.onescol && j == 0) ? 1.0 : rr_svi_xval(c, row, j - c.onescol);
        }
    }
    __syncthreads();
    if (k == 0)   // Phi does not depend on the component: kernel C reads it back instead of forming it again
        for (int e = tid; e < M * w; e += SW_THREADS) a.Phi[(size_t)(e / w) * F + sw_col<GM>(c, it, e % w)] = Phi[(e / w) * wp + e % w];
    // the item's partial of fs[k, l, r] = sum_col (m + sqrt(C) e)[l][col] Phi[r][col]
    double *fsp = a.fsp + ((size_t)ii * K + k) * L * M;
    for (int o = tid; o < L * M; o += SW_THREADS) {
        const int l = o / M, r = o % M;
        double acc = 0.0;
        for (int cc = 0; cc < w; ++cc) acc = fma(fma(sk[cc], (double)Ef[l * w + cc], mk[cc]), Phi[r * wp + cc], acc);
        fsp[o] = acc;
    }
    // the item's partial of q[k][l] = sum_f log(C_fk + C_fl) + (m_fk - m_fl)^2 / (C_fk + C_fl): one wave per l   glm.py:697-712
    for (int l = wave; l < K; l += SW_WAVES) {
        double acc = 0.0;
        for (int cc = lane; cc < w; cc += 64) {
            const int64_t col = sw_col<GM>(c, it, cc);
            const double dc = xC[col * K + k] + xC[col * K + l];
            const double dm = xm[col * K + k] - xm[col * K + l];
            acc += log(dc) + dm * dm / dc;
        }
        acc = rr_svi_wave_sum(acc);
        if (lane == 0) a.qp[((size_t)ii * K + k) * K + l] = acc;
    }
    if (wave == 0) {   // and of sum (m^2 + C) over the child's rows of component k
        double acc = 0.0;
        for (int cc = lane; cc < w; cc += 64) acc += mk[cc] * mk[cc] + sk[cc] * sk[cc];
        acc = rr_svi_wave_sum(acc);
        if (lane == 0) a.Rp[(size_t)ii * K + k] = acc;
    }
}

// ---- B ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(SW_THREADS) rr_glm_sviw_b_kernel(const SwArgs a) {
#pragma clang fp contract(off)
    __shared__ double redm[8];
    ldsd *red = (ldsd *)redm;
    const int tid = threadIdx.x, bx = blockIdx.x, k = blockIdx.y, K = a.K, L = a.L, M = a.M, LM = L * M;
    RR_DEV_ASSERT(bx < a.nbx && k < K);
    const int64_t fk = (int64_t)a.F * K;
    const double ivar = a.n_lik ? 1.0 / a.xin[2 * fk + a.nkids] : 0.0;
    const int o = bx * SW_THREADS + tid;
    double ll = 0.0;
    if (o < LM) {
        const int r = o % M;
        double fs = 0.0;
        for (int ii = 0; ii < a.nitems; ++ii) fs += a.fsp[((size_t)ii * K + k) * LM + o];
        const int64_t row = a.idx[r];
        RR_DEV_ASSERT(row >= 0 && row < a.N);
        const double y = a.y_f64 ? ((const double *)a.y)[row] : (double)((const float *)a.y)[row];
        double n = 0.0;
        if (a.rowarg) n = a.y_f64 ? ((const double *)a.rowarg)[row] : (double)((const float *)a.rowarg)[row];
        double df;
        rr_svi_lik(a.lik, fs, y, n, ivar, df, ll);
        a.dfs[(size_t)k * LM + o] = df;
    }
    ll = sw_block_sum(ll, red);
    if (tid == 0) a.llp[(size_t)k * a.nbx + bx] = ll;
    if (bx == 0) {
        if (tid < K) {
            double q = 0.0;
            for (int ii = 0; ii < a.nitems; ++ii) q += a.qp[((size_t)ii * K + k) * K + tid];
            a.qf[k * K + tid] = q;
        } else if (tid < K + a.nkids) {
            const SwChild &c = a.kid[tid - K];
            RR_DEV_ASSERT(c.item0 >= 0 && c.item0 + c.nitems <= a.nitems);
            double R = 0.0;
            for (int ii = c.item0; ii < c.item0 + c.nitems; ++ii) R += a.Rp[(size_t)ii * K + k];
            a.Rk[(tid - K) * K + k] = R;
        }
    }
}

// ---- C ------------------------------------------------------------------------------------------------------------------
template <bool GM>
__global__ void __launch_bounds__(SW_THREADS) rr_glm_sviw_c_kernel(const SwArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double sm[];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, ii = blockIdx.x, k = blockIdx.y;
    const int K = a.K, F = a.F, L = a.L, M = a.M;
    RR_DEV_ASSERT(ii < a.nitems && k < K);
    const SwItem it = a.items[ii];
    const SwChild &c = a.kid[it.child];
    sw_check_item<GM>(a, c, it);
    // (rff: an item of [cos | sin] column pairs -- a random Fourier child's or, gm, a spectral-mixture component's two pairs)
    const bool gm = GM && c.kind == RR_SGD_CHILD_GM, rff = gm || c.kind == RR_SGD_CHILD_RFF;
    const SwLay s = sw_layout<GM>(gm ? 2 : rff, it.cnt, c.d, K, L, M, 1);
    const int w = s.w, wp = s.wp, cnt = it.cnt;
    ldsd *b = (ldsd *)sm;
    ldsd *Xb = b + s.Xb, *Wl = b + s.Wl, *Phi = b + s.Phi, *mk = b + s.mk, *sk = b + s.sk, *dfs = b + s.dfs, *Q = b + s.Q, *T = b + s.T,
         *Dr = b + s.Dr, *q = b + s.q, *logz = b + s.logz, *alpha = b + s.alpha, *red = b + s.red;
    ldsf *Ef = (ldsf *)(b + s.Ef);
    const int64_t fk = (int64_t)F * K;
    const double *xm = a.xin, *xC = a.xin + fk, *xs = a.xin + 2 * fk;
    for (int o = tid; o < L * M; o += SW_THREADS) dfs[o] = a.dfs[(size_t)k * L * M + o];
    for (int cc = tid; cc < w; cc += SW_THREADS) {
        const int col = sw_col<GM>(c, it, cc);
        mk[cc] = xm[(int64_t)col * K + k];
        sk[cc] = sqrt(xC[(int64_t)col * K + k]);
    }
    for (int e = tid; e < M * w; e += SW_THREADS) Phi[(e / w) * wp + e % w] = a.Phi[(size_t)(e / w) * F + sw_col<GM>(c, it, e % w)];
    for (int o = tid; o < K * K; o += SW_THREADS) q[o] = a.qf[o];
    if (rff) {
        sw_gather(a, c, Xb);
        for (int e = tid; e < c.d * cnt; e += SW_THREADS) Wl[e] = c.W[(size_t)(e / cnt) * c.n + it.j0 + e % cnt];
        sw_draws<GM>(a, c, it, k, w, Ef);
    }
    __syncthreads();
    rr_svi_logz(a.F, a.K, q, logz);
    __syncthreads();
    if (tid < K) {
        const double lN = -0.5 * ((double)F * 1.8378770664093453 + q[tid * K + k]);
        alpha[tid] = exp(lN - logz[k]) + exp(lN - logz[tid]);
    }
    // D_r = sum_l dfs[l][r]; Q[r][j] = sum_l dfs[l][r] e[l][j]: the only sums over the samples the gradients need
    if (tid < M) {
        double acc = 0.0;
        for (int l = 0; l < L; ++l) acc += dfs[l * M + tid];
        Dr[tid] = acc;
    }
    if (rff) {
        for (int o = tid; o < M * w; o += SW_THREADS) {
            const int r = o / w, cc = o % w;
            double acc = 0.0;
            for (int l = 0; l < L; ++l) acc = fma(dfs[l * M + r], (double)Ef[l * w + cc], acc);
            Q[o] = acc;
        }
    }
    __syncthreads();
    //   Edm[j] = sum_r D_r Phi[r][j] / L;  EdC[j] = sum_r Q[r][j] Phi[r][j] / (L sk[j])           glm.py:308-310
    // then the gradient of (m, C)[col][k], the log trick's chain rule, bounds, updater, clip          glm.py:252-256, sgd.py:404-420
    const double reg = xs[it.child];
    double n2 = 0.0;
    for (int p = tid; p < 2 * w; p += SW_THREADS) {
        const int cov = p >= w, cc = cov ? p - w : p;
        const int64_t col = sw_col<GM>(c, it, cc);
        double ed = 0.0;
        if (!cov) {
            for (int r = 0; r < M; ++r) ed = fma(Dr[r], Phi[r * wp + cc], ed);
            ed = ed / L;
        } else if (rff) {
            for (int r = 0; r < M; ++r) ed = fma(Q[r * w + cc], Phi[r * wp + cc], ed);
            ed = ed / (L * sk[cc]);
        } else {
            // a linear child keeps neither Q nor its draws: sum_r Q[r][j] Phi[r][j] = sum_l e[l][j] (sum_r dfs[l][r] Phi[r][j]), each
            // draw read (or made) once, by the one thread that owns column j
            for (int l = 0; l < L; ++l) {
                double t = 0.0;
                for (int r = 0; r < M; ++r) t = fma(dfs[l * M + r], Phi[r * wp + cc], t);
                const uint64_t ctr = ((uint64_t)k * (uint64_t)L + (uint64_t)l) * (uint64_t)F + (uint64_t)col;
                ed = fma((double)(a.E ? a.E[ctr] : rr_svi_draw(a.stepkey, ctr)), t, ed);
            }
            ed = ed / (L * sk[cc]);
        }
        const double mkv = xm[col * K + k], Ck = xC[col * K + k];
        double mix = 0.0;
        for (int l = 0; l < K; ++l) {
            const double ic = 1.0 / (Ck + xC[col * K + l]);
            const double dm = mkv - xm[col * K + l];
            const double e = dm * ic;
            mix += (cov ? ic - e * e : ic * dm) * alpha[l];
        }
        double g;
        if (!cov) g = -((a.bmag * ed - mkv / reg + mix) / K);
        else g = -((a.bmag * ed - 1.0 / reg + mix) / (2 * K));
        const int64_t gi = (cov ? fk : 0) + col * K + k;
        RR_DEV_ASSERT(gi >= 0 && gi < 2 * fk);
        const bool lg = a.islog[gi] != 0;
        if (lg) g *= cov ? Ck : mkv;
        n2 += g * g;
        double s1 = a.s1[gi], s2 = a.s2[gi];
        const double zn = rr_svi_update(a, a.z[gi], g, a.lower[gi], a.upper[gi], s1, s2, a.b1t, a.b2t);
        a.s1[gi] = s1;
        a.s2[gi] = s2;
        a.z[gi] = zn;
        a.xout[gi] = lg ? exp(zn) : zn;
    }
    n2 = sw_block_sum(n2, red);
    if (tid == 0) a.n2p[(size_t)ii * K + k] = n2;
    if (!rff) return;
    if (gm) {
        // T+-[r][j] = EdPhi_sin+- Phi_cos+- - EdPhi_cos+- Phi_sin+- over the + and the - pair of blocks; slot mean_i takes
        // sum_{r, j} x_ri (T- - T+)[r][j], slot l_i sum_{r, j} V_ij x_ri (T+ + T-)[r][j] (the factor 1 / l_i^2 in kernel D): means first,
        // then length scales -- rr_svi.hip's formulas for the component (basis_functions.py:1477-1537)
        const double sc = 1.0 / ((double)L * K);
        ldsd *Tp = T, *Tm = T + M * cnt;
        for (int o = tid; o < 2 * M * cnt; o += SW_THREADS) {
            const int blk = o / (M * cnt), e = o % (M * cnt), r = e / cnt, jc = 2 * blk * cnt + e % cnt, js = jc + cnt;
            const double epc = (mk[jc] * Dr[r] + sk[jc] * Q[r * w + jc]) * sc;
            const double eps = (mk[js] * Dr[r] + sk[js] * Q[r * w + js]) * sc;
            T[o] = eps * Phi[r * wp + jc] - epc * Phi[r * wp + js];
        }
        __syncthreads();
        for (int h = wave; h < 2 * c.d; h += SW_WAVES) {
            const bool mean = h < c.d;
            const int i = mean ? h : h - c.d;
            RR_DEV_ASSERT(h < c.n_ls && c.ls0 + h < a.n_ls && h < a.maxls && i < c.d);
            double acc = 0.0;
            for (int o = lane; o < M * cnt; o += 64) {
                const int r = o / cnt, j = o % cnt;
                if (mean) acc = fma(Xb[r * c.d + i], Tm[o] - Tp[o], acc);
                else acc = fma(Wl[i * cnt + j] * Xb[r * c.d + i], Tp[o] + Tm[o], acc);
            }
            acc = rr_svi_wave_sum(acc);
            if (lane == 0) a.glsp[((size_t)ii * K + k) * a.maxls + h] = acc;
        }
        return;
    }
    // the item's share of -(EdPhi o dPhi_i).sum() of this component: W[i, :] . T[i, :] (the factor 1 / l_i^2 in kernel D) with
    // T = X^T (E_s o P_c - E_c o P_s), EdPhi[r][j] = (mk[j] D_r + sk[j] Q[r][j]) / (L K); the isotropic parameter takes input
    // dimension 0 only, as the reference does (basis_functions.py:896)
    const double sc = 1.0 / ((double)L * K);
    for (int o = tid; o < M * cnt; o += SW_THREADS) {
        const int r = o / cnt, j = o % cnt, js = cnt + j;
        const double epc = (mk[j] * Dr[r] + sk[j] * Q[r * w + j]) * sc;
        const double eps = (mk[js] * Dr[r] + sk[js] * Q[r * w + js]) * sc;
        T[o] = eps * Phi[r * wp + j] - epc * Phi[r * wp + js];
    }
    __syncthreads();
    for (int i = wave; i < c.n_ls; i += SW_WAVES) {
        RR_DEV_ASSERT(i < c.d && c.ls0 + i < a.n_ls && i < a.maxls);
        double acc = 0.0;
        for (int o = lane; o < M * cnt; o += 64) {
            const int r = o / cnt, j = o % cnt;
            acc = fma(Wl[i * cnt + j] * Xb[r * c.d + i], T[o], acc);
        }
        acc = rr_svi_wave_sum(acc);
        if (lane == 0) a.glsp[((size_t)ii * K + k) * a.maxls + i] = acc;
    }
}

// ---- D ------------------------------------------------------------------------------------------------------------------
template <bool GM>
__global__ void __launch_bounds__(SW_THREADS) rr_glm_sviw_d_kernel(const SwArgs a) {
#pragma clang fp contract(off)
    __shared__ double qm[SW_MAXK * SW_MAXK], logzm[SW_MAXK], llm[SW_MAXK], Rcm[SW_MAXCHILD], glsm[SW_MAXCHILD * SW_MAXD], redm[8];
    ldsd *q = (ldsd *)qm, *logz = (ldsd *)logzm, *llk = (ldsd *)llm, *Rc = (ldsd *)Rcm, *gls = (ldsd *)glsm, *red = (ldsd *)redm;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, K = a.K, F = a.F, L = a.L, M = a.M, nk = a.nkids, ns = a.ns;
    const int64_t fk = (int64_t)F * K;
    const double *xs = a.xin + 2 * fk;
    RR_DEV_ASSERT(K <= SW_MAXK && nk <= SW_MAXCHILD && a.n_ls <= SW_MAXCHILD * SW_MAXD && ns == nk + a.n_lik + a.n_ls);
    for (int o = tid; o < K * K; o += SW_THREADS) q[o] = a.qf[o];
    if (tid < K) {   // sum of the log-likelihood terms of component tid (Gaussian: of the squared errors), block by block
        double acc = 0.0;
        for (int bx = 0; bx < a.nbx; ++bx) acc += a.llp[(size_t)tid * a.nbx + bx];
        llk[tid] = acc;
    } else if (tid >= 64 && tid < 64 + nk) {
        double acc = 0.0;
        for (int j = 0; j < K; ++j) acc += a.Rk[(tid - 64) * K + j];
        Rc[tid - 64] = acc;
    }
    __syncthreads();
    rr_svi_logz(a.F, a.K, q, logz);
    __syncthreads();
    // the batch's f-independent part of loglike per latent sample (the log-factorial terms)
    double lc = 0.0;
    if (tid < M && a.lconst) {
        const int64_t row = a.idx[tid];
        RR_DEV_ASSERT(row >= 0 && row < a.N);
        lc = a.lconst[row];
    }
    lc = sw_block_sum(lc, red);
    double n2 = 0.0;
    if (!a.objective_only) {
        // the length scales' contractions: per slot the (item, component) partials of its child, one wave per slot
        for (int h = wave; h < a.n_ls; h += SW_WAVES) {
            int ci = 0;
            while (ci + 1 < nk && !(h >= a.kid[ci].ls0 && h < a.kid[ci].ls0 + a.kid[ci].n_ls)) ++ci;
            const SwChild &c = a.kid[ci];
            const int i = h - c.ls0;
            // (a spectral-mixture component's 2 d slots sit in glsp as they do in z: means, then length scales)
            RR_DEV_ASSERT(i >= 0 && i < c.n_ls && i < a.maxls && c.item0 >= 0 && c.item0 + c.nitems <= a.nitems);
            double acc = 0.0;
            for (int e = lane; e < K * c.nitems; e += 64)
                acc += a.glsp[((size_t)(c.item0 + e % c.nitems) * K + e / c.nitems) * a.maxls + i];
            acc = rr_svi_wave_sum(acc);
            if (lane == 0) gls[h] = acc;
        }
        for (int e = tid; e < a.nitems * K; e += SW_THREADS) n2 += a.n2p[e];
        n2 = sw_block_sum(n2, red);
    }
    __syncthreads();
    double n2s = 0.0;
    if (!a.objective_only) {
        for (int p = tid; p < ns; p += SW_THREADS) {
            double g;
            if (p < nk) {  // dreg of the child's slice (glm.py:265-268)
                const double iL = 1.0 / xs[p];
                g = -(0.5 * (Rc[p] * (iL * iL) / K - (double)a.kid[p].width * iL));
            } else if (p < nk + a.n_lik) {  // Gaussian variance (likelihoods.py:370-396)
                const double iv = 1.0 / xs[p];
                double sm2 = 0.0;
                for (int j = 0; j < K; ++j) sm2 += 0.5 * (llk[j] * iv * iv - iv * (double)M * L) / L;
                g = 0.0 - sm2 / K;
            } else {
                const double l = xs[p];
                g = gls[p - nk - a.n_lik] / (1.0 * (l * l));
                if (GM) {   // the slot's factor is 1 / l^2 for a length scale, 1 for a spectral-mixture mean (any sign, never a divisor)
                    const int h = p - nk - a.n_lik;
                    bool mean = false;
                    for (int ci = 0; ci < nk; ++ci)
                        mean = mean || (a.kid[ci].kind == RR_SGD_CHILD_GM && h >= a.kid[ci].ls0 && h < a.kid[ci].ls0 + a.kid[ci].d);
                    if (mean) g = gls[h];
                }
            }
            const int64_t gi = 2 * fk + p;
            const bool lg = a.islog[gi] != 0;
            if (lg) g *= xs[p];
            n2s += g * g;
            double s1 = a.s1[gi], s2 = a.s2[gi];
            const double zn = rr_svi_update(a, a.z[gi], g, a.lower[gi], a.upper[gi], s1, s2, a.b1t, a.b2t);
            a.s1[gi] = s1;
            a.s2[gi] = s2;
            a.z[gi] = zn;
            a.xout[gi] = lg ? exp(zn) : zn;
        }
        n2s = sw_block_sum(n2s, red);
    }
    if (wave == 0) {   // the record: |g| (sgd.py:399) and -ELBO (glm.py:285-292)
        double ell = 0.0, part = 0.0;
        const double ivar = a.n_lik ? 1.0 / xs[nk] : 0.0;
        for (int j = lane; j < K; j += 64) ell += (a.n_lik ? -0.5 * llk[j] * ivar : llk[j]) / L;
        double llc = lc;
        if (a.n_lik) llc = -0.5 * log(2.0 * 3.141592653589793 * xs[nk]) * (double)M;
        ell = rr_svi_wave_sum(ell) + llc * K;
        for (int ci = lane; ci < nk; ci += 64) {
            const double reg = xs[ci];
            part += -0.5 * K * ((double)a.kid[ci].width * log(reg)) - 0.5 * (Rc[ci] / reg);
        }
        for (int j = lane; j < K; j += 64) part -= logz[j];
        part = rr_svi_wave_sum(part);
        const double elbo = (ell * a.bmag - 0.5 * F * K * 1.8378770664093453 + part + log((double)K)) / K;
        if (lane == 0) {
            *a.obj = -elbo;
            if (a.norm) *a.norm = sqrt(n2 + n2s);
        }
    }
}

// x = from_log(z) of every coordinate (create, set_start: not part of a step)
__global__ void __launch_bounds__(SW_THREADS) rr_glm_sviw_x_kernel(const double *z, const unsigned char *islog, double *x, int64_t np) {
    const int64_t p = (int64_t)blockIdx.x * SW_THREADS + threadIdx.x;
    if (p < np) x[p] = islog[p] ? exp(z[p]) : z[p];
}

// ---- the one place that decides the split -------------------------------------------------------------------------------
// width: the largest count of frequencies <= SW_ITEM_DEFAULT (RR_SVIW_ITEM replaces that cap) whose item fits the LDS budget for
// every random Fourier child; a linear child is one item whatever its width.  gmok (rr_glm_sviwgm_*): spectral-mixture children
// too, cut the same way with a width of their own -- the largest count <= SW_ITEM_GM_DEFAULT (RR_SVIW_ITEM replaces that cap as
// well) whose item fits for every such child.  Returns the number of items, or -1 when an item cannot fit (or a child is of
// another kind); items (cap triples) may be null.  info: (items, width, worst item's bytes, budget, spectral-mixture width).
static int sw_kind_pairs(int kind) { return kind == RR_SGD_CHILD_GM ? 2 : (kind == RR_SGD_CHILD_RFF ? 1 : 0); }

static int sw_plan(int n_children, const int *kind, const int *n, const int *d, int K, int L, int M, int cap, int *items, int64_t info[5],
                   bool gmok = false) {
    int width = SW_ITEM_DEFAULT, gwidth = SW_ITEM_GM_DEFAULT;
    const char *env = getenv("RR_SVIW_ITEM");
    if (env && atoi(env) >= 1) width = gwidth = atoi(env);
    size_t worst = 0;
    for (int c = 0; c < n_children; ++c) {
        if (kind[c] == RR_SGD_CHILD_RFF || (gmok && kind[c] == RR_SGD_CHILD_GM)) {
            if (n[c] < 1 || d[c] < 1) return -1;
            const int pairs = sw_kind_pairs(kind[c]);
            int &wd = pairs == 2 ? gwidth : width;
            int wc = std::min(wd, n[c]);
            while (wc >= 1 && sw_item_bytes(pairs, wc, d[c], K, L, M) > SW_LDS_BUDGET) --wc;
            if (wc < 1) return -1;
            if (wc < std::min(wd, n[c])) wd = wc;
        } else if (kind[c] == RR_SGD_CHILD_LINEAR) {
            if (n[c] < 1 || sw_item_bytes(0, n[c], d[c], K, L, M) > SW_LDS_BUDGET) return -1;
        } else {
            return -1;
        }
    }
    int ni = 0;
    for (int c = 0; c < n_children; ++c) {
        const int pairs = sw_kind_pairs(kind[c]), wd = pairs == 2 ? gwidth : width;
        for (int j0 = 0; j0 < n[c]; j0 += pairs ? wd : n[c]) {
            const int cnt = pairs ? std::min(wd, n[c] - j0) : n[c];
            worst = std::max(worst, sw_item_bytes(pairs, cnt, d[c], K, L, M));
            if (items && ni < cap) {
                items[3 * ni] = c;
                items[3 * ni + 1] = j0;
                items[3 * ni + 2] = cnt;
            }
            ++ni;
        }
    }
    if (info) {
        info[0] = ni;
        info[1] = width;
        info[2] = (int64_t)worst;
        info[3] = SW_LDS_BUDGET;
        info[4] = gwidth;
    }
    return ni;
}

}  // namespace

struct rr_glm_sviw {
    rr_ctx *ctx = nullptr;
    SwArgs a;
    SwChild hkid[SW_MAXCHILD];
    SwChild *dkid = nullptr;
    SwItem *ditems = nullptr;
    std::vector<double *> dW;
    RrSviState st;
    double *xbuf[2] = {nullptr, nullptr};
    size_t lds_bytes = 0;
    bool gm = false;   // a spectral-mixture child among them: the kernels' <true> instances
};

static void sw_free(rr_glm_sviw *o) {
    rr_svi_state_free(o->st);
    void *q[] = {o->dkid, o->ditems, o->xbuf[0], o->xbuf[1], o->a.Phi, o->a.fsp, o->a.qp, o->a.Rp, o->a.dfs, o->a.llp, o->a.qf, o->a.Rk,
                 o->a.n2p, o->a.glsp};
    for (void *v : q)
        if (v) (void)hipFree(v);
    for (double *w : o->dW)
        if (w) (void)hipFree(w);
    delete o;
}

static void sw_form_x(rr_glm_sviw *o) {
    const int64_t np = o->a.np;
    hipLaunchKernelGGL(rr_glm_sviw_x_kernel, dim3((unsigned)((np + SW_THREADS - 1) / SW_THREADS)), dim3(SW_THREADS), 0, o->ctx->stream,
                       (const double *)o->st.z, (const unsigned char *)o->st.islog, o->xbuf[o->st.t & 1], np);
}

extern "C" {

int rr_glm_sviw_supported(int F, int K, int L, int M, int n_children, int dsum, int n_ls) {
    if (F < 1 || F > SW_MAXF || K < 1 || K > SW_MAXK || L < 1 || L > SW_MAXL || M < 1 || M > SW_MAXM) return 0;
    if (n_children < 1 || n_children > SW_MAXCHILD || F < n_children || dsum < 0 || dsum > SW_MAXCHILD * SW_MAXD) return 0;
    if (n_ls < 0 || n_ls > SW_MAXCHILD * SW_MAXD) return 0;
    // the widest child the inputs allow: one random Fourier child and one linear child over min(dsum, 128) columns must both fit
    const int d = std::max(1, std::min(dsum, SW_MAXD));
    const int kind[2] = {RR_SGD_CHILD_RFF, RR_SGD_CHILD_LINEAR}, n[2] = {std::max(1, F / 2), std::min(F, d + 1)}, dd[2] = {d, d};
    int64_t info[5];
    if (sw_plan(2, kind, n, dd, K, L, M, 0, nullptr, info) < 1) return 0;
    // the partials of fs: (items, K, L, M) doubles
    const int64_t items = (F / 2 + info[1] - 1) / info[1] + n_children;
    if (items * K * L * M * 8 > SW_SCRATCH_MAX) return 0;
    // The upper edge in minibatch x F, from the measured per-step times (docs/KERNELS.md 3.48: MI355X, K L = 500, d = 21, F = 512
    // ... 16384, minibatches of 10, 32 and 64 rows): the chain costs ~55 + 0.005 F + 7.4e-4 M F (K L / 500) us, the step-per-call
    // loop ~150 + 0.025 F us whatever the minibatch.  In range is what the chain wins by 1.25 x on that model: every measured
    // shape inside won by 2.2 x or more, the two that won by 1.2 x (64 rows at F = 2048, 32 at F = 16384) and the one that lost
    // (64 at F = 16384) are outside.  Nothing routes to a slower loop.
    const double wide_us = 55.0 + 0.005 * F + 7.4e-4 * (double)M * F * ((double)K * L / 500.0);
    const double step_us = 150.0 + 0.025 * F;
    return 1.25 * wide_us <= step_us ? 1 : 0;
}

int rr_glm_sviwgm_supported(int F, int K, int L, int M, int n_children, int dsum, int n_ls, int gm_cols) {
    if (gm_cols == 0) return rr_glm_sviw_supported(F, K, L, M, n_children, dsum, n_ls);
    if (F < 1 || F > SW_MAXF || K < 1 || K > SW_MAXK || L < 1 || L > SW_MAXL || M < 1 || M > SW_MAXM) return 0;
    if (n_children < 1 || n_children > SW_MAXCHILD || F < n_children || dsum < 0 || dsum > SW_MAXCHILD * SW_MAXD) return 0;
    if (n_ls < 0 || n_ls > SW_MAXCHILD * SW_MAXD || gm_cols < 4 || gm_cols > F || gm_cols % 4) return 0;
    // the widest children the inputs allow: one spectral-mixture component of all gm_cols columns, one random Fourier child of
    // the rest and one linear child, each over min(dsum, 128) columns of X, must fit
    const int d = std::max(1, std::min(dsum, SW_MAXD));
    const int kind[3] = {RR_SGD_CHILD_GM, RR_SGD_CHILD_LINEAR, RR_SGD_CHILD_RFF};
    const int n[3] = {gm_cols / 4, std::min(F, d + 1), std::max(1, (F - gm_cols) / 2)}, dd[3] = {d, d, d};
    int64_t info[5];
    if (sw_plan(F - gm_cols >= 2 ? 3 : 2, kind, n, dd, K, L, M, 0, nullptr, info, true) < 1) return 0;
    const int64_t items = (gm_cols / 4 + info[4] - 1) / info[4] + ((F - gm_cols) / 2 + info[1] - 1) / info[1] + 2 * (int64_t)n_children;
    if (items * K * L * M * 8 > SW_SCRATCH_MAX) return 0;
    // The upper edge, as rr_glm_sviw_supported's: in range is what the chain wins by 1.25 x on a model fitted to the measured
    // per-step times (docs/KERNELS.md 3.50: MI355X, K L = 500, Xdim = 4, one to eight components, F = 128 ... 4096, minibatches
    // of 10, 32 and 64 rows).  Both sides err against the chain: its time ~58 + 0.0146 F + 2.5e-3 (M - 10) F us is the measured
    // one at 10 rows up to F = 1024 and at 32 rows, and above it at F = 4096 (by 17 %) and at 64 rows (by 24 %); the F terms grow
    // with K L beyond 500 and do not shrink below it (not measured).  The step-per-call loop took 125 + 16 per component +
    // 0.035 F us or more at 10 rows and more at larger minibatches; the number of components is not known here, so ONE is
    // assumed and the other columns are priced as random Fourier columns (3.48).  Every measured shape inside won by 2.5 x or more.
    const double kl = std::max(1.0, (double)K * L / 500.0);
    const double wide_us = 58.0 + (0.0146 * F + 2.5e-3 * (double)std::max(M - 10, 0) * F) * kl;
    const double step_us = 141.0 + 0.025 * F + 0.010 * gm_cols;
    return 1.25 * wide_us <= step_us ? 1 : 0;
}

int rr_glm_sviwgm_plan(int n_children, const int *kind, const int *n, const int *d, int K, int L, int M, int cap, int *items,
                       int64_t info[5]) {
    RR_REQUIRE(kind != nullptr && n != nullptr && d != nullptr && info != nullptr && n_children >= 1 && n_children <= SW_MAXCHILD &&
               K >= 1 && K <= SW_MAXK && L >= 1 && M >= 1 && cap >= 0, "rr_glm_sviwgm_plan: bad argument");
    for (int c = 0; c < n_children; ++c)
        RR_REQUIRE(kind[c] == RR_SGD_CHILD_RFF || kind[c] == RR_SGD_CHILD_LINEAR || kind[c] == RR_SGD_CHILD_GM,
                   "rr_glm_sviwgm_plan: child %d: kind %d is not taken by the wide loop (random Fourier, spectral-mixture and linear "
                   "children only)", c, kind[c]);
    if (sw_plan(n_children, kind, n, d, K, L, M, cap, items, info, true) < 1) {
        rr_set_error("rr_glm_sviwgm_plan: no item of this shape fits %d bytes of LDS (K = %d, nsamples = %d, minibatch = %d)",
                     SW_LDS_BUDGET, K, L, M);
        return RR_ERR_UNSUPPORTED;
    }
    return RR_OK;
}

int rr_glm_sviw_plan(int n_children, const int *kind, const int *n, const int *d, int K, int L, int M, int cap, int *items,
                     int64_t info[4]) {
    RR_REQUIRE(kind != nullptr && n != nullptr && d != nullptr && info != nullptr && n_children >= 1 && n_children <= SW_MAXCHILD &&
               K >= 1 && K <= SW_MAXK && L >= 1 && M >= 1 && cap >= 0, "rr_glm_sviw_plan: bad argument");
    for (int c = 0; c < n_children; ++c)
        RR_REQUIRE(kind[c] == RR_SGD_CHILD_RFF || kind[c] == RR_SGD_CHILD_LINEAR, "rr_glm_sviw_plan: child %d: kind %d is not taken by "
                   "the wide loop (random Fourier and linear children only)", c, kind[c]);
    int64_t inf[5];
    const int ni = sw_plan(n_children, kind, n, d, K, L, M, cap, items, inf);
    for (int i = 0; i < 4; ++i) info[i] = ni < 1 ? 0 : inf[i];
    if (ni < 1) {
        rr_set_error("rr_glm_sviw_plan: no item of this shape fits %d bytes of LDS (K = %d, nsamples = %d, minibatch = %d)",
                     SW_LDS_BUDGET, K, L, M);
        return RR_ERR_UNSUPPORTED;
    }
    return RR_OK;
}

// gmok: rr_glm_sviwgm_create -- spectral-mixture children too; rr_glm_sviw_create refuses them as it always did
static int sw_create(bool gmok, rr_ctx *ctx, int n_children, const rr_glm_sgd_child *children, const void *const *dX, const int *x_dtype,
                     const int64_t *ldx, int64_t N, const void *dy, const void *drowarg, const double *dlconst, int dtype, int K, int L,
                     int M, int lik, int n_lik, const double *z0, const double *lower, const double *upper, const unsigned char *is_log,
                     int updater, const double *upd_par, int64_t maxiter, double bmag, rr_glm_sviw **out) {
    const char *who = gmok ? "rr_glm_sviwgm_create" : "rr_glm_sviw_create";
    const int rc = rr_svi_check_create(who, SW_MAXCHILD, SW_MAXK, ctx, n_children, children, dX, x_dtype, ldx, N, dy, drowarg, dtype, K, L,
                                       M, lik, n_lik, z0, lower, upper, is_log, updater, upd_par, maxiter, (void **)out);
    if (rc != RR_OK) return rc;
    for (int s = 0; s < n_children; ++s) {
        if (gmok)
            RR_REQUIRE(children[s].kind == RR_SGD_CHILD_RFF || children[s].kind == RR_SGD_CHILD_LINEAR || children[s].kind == RR_SGD_CHILD_GM,
                       "%s: child %d: kind %d is not taken by the wide loop (random Fourier, spectral-mixture and linear children only)",
                       who, s, children[s].kind);
        else
            RR_REQUIRE(children[s].kind == RR_SGD_CHILD_RFF || children[s].kind == RR_SGD_CHILD_LINEAR,
                       "%s: child %d: kind %d is not taken by the wide loop (random Fourier and linear children only)", who, s, children[s].kind);
    }
    RR_CHECK_HIP(hipSetDevice(ctx->device));
    rr_glm_sviw *o = new rr_glm_sviw();
    o->ctx = ctx;
    SwArgs &a = o->a;
    memset(&a, 0, sizeof a);
    memset(o->hkid, 0, sizeof o->hkid);
    int col = 0, nls = 0, dsum = 0, maxls = 1, gm_cols = 0;
    int pk[SW_MAXCHILD], pn[SW_MAXCHILD], pd[SW_MAXCHILD];
    for (int s = 0; s < n_children; ++s) {
        const rr_glm_sgd_child &k = children[s];
        SwChild &c = o->hkid[s];
        c.kind = k.kind;
        c.col0 = col;
        c.ls0 = nls;
        c.X = dX[s];
        c.ldx = ldx[s];
        c.x_f64 = x_dtype[s] == RR_F64;
        bool ok = dX[s] != nullptr && (x_dtype[s] == RR_F32 || x_dtype[s] == RR_F64);
        const bool gm = k.kind == RR_SGD_CHILD_GM;
        if (gm) {   // rr_glm_svi_create_gm's child contract (basis_functions.py:1386-1562 through the chain's dense equivalent)
            rr_basis *b = k.basis;
            if (!(ok && b != nullptr && b->kind == RR_KIND_RFF && b->ctx == ctx && !b->large && b->d >= 1 && b->d <= SW_MAXD && b->n >= 1 &&
                  k.n_ls == 2 * b->d && (int)b->W.size() == b->d * b->n)) {
                sw_free(o);
                rr_set_error("%s: child %d: a spectral-mixture child (RR_SGD_CHILD_GM) needs the dense random Fourier equivalent of its "
                             "chain on this context, Xdim <= %d, n_ls = 2 Xdim coordinates [mean | length scales] (n_ls=%d, Xdim=%d) and "
                             "its resident rows", who, s, SW_MAXD, k.n_ls, b != nullptr && b->kind == RR_KIND_RFF ? b->d : -1);
                return RR_ERR_INVALID;
            }
        }
        if (ok && (k.kind == RR_SGD_CHILD_RFF || gm)) {
            rr_basis *b = k.basis;
            ok = gm || (b != nullptr && b->kind == RR_KIND_RFF && b->ctx == ctx && b->d >= 1 && b->d <= SW_MAXD && b->n >= 1 &&
                        (k.n_ls == 1 || k.n_ls == b->d) && (int)b->W.size() == b->d * b->n);
            if (ok) {
                c.d = b->d; c.n = b->n; c.n_ls = k.n_ls; c.width = (gm ? 4 : 2) * b->n; c.onescol = 0;
                gm_cols += gm ? c.width : 0;
                double *w = rr_svi_upload_w(b);
                if (!w) {
                    sw_free(o);
                    rr_set_error("%s: device allocation failed", who);
                    return RR_ERR_OOM;
                }
                o->dW.push_back(w);
                c.W = w;
                pn[s] = c.n;
            }
        } else if (ok) {
            ok = k.d >= 1 && k.d <= SW_MAXD && k.n_ls == 0;
            c.d = k.d; c.n = 0; c.n_ls = 0; c.onescol = k.onescol ? 1 : 0; c.width = k.d + c.onescol;
            pn[s] = c.width;
        }
        if (!ok) {
            sw_free(o);
            rr_set_error("%s: child %d: a random Fourier basis of this context with Xdim <= %d and 1 or Xdim length scales, or a "
                         "linear child with 1 <= d <= %d columns, and its resident rows", who, s, SW_MAXD, SW_MAXD);
            return RR_ERR_INVALID;
        }
        pk[s] = c.kind;
        pd[s] = c.d;
        maxls = std::max(maxls, c.n_ls);
        col += c.width;
        nls += c.n_ls;
        dsum += c.d;
    }
    a.nkids = n_children; a.F = col; a.K = K; a.L = L; a.M = M; a.lik = lik; a.n_lik = n_lik; a.n_ls = nls; a.maxls = maxls;
    a.ns = n_children + n_lik + nls; a.updater = updater; a.y_f64 = dtype == RR_F64; a.N = N;
    a.np = 2 * (int64_t)col * K + a.ns;
    a.y = dy; a.rowarg = drowarg; a.lconst = dlconst; a.bmag = bmag;
    a.nbx = (L * M + SW_THREADS - 1) / SW_THREADS;
    for (int i = 0; i < 4; ++i) a.up[i] = upd_par[i];
    int64_t info[5] = {0, 0, 0, 0, 0};
    const int ni = rr_glm_sviwgm_supported(a.F, K, L, M, n_children, dsum, nls, gm_cols)
                       ? sw_plan(n_children, pk, pn, pd, K, L, M, 0, nullptr, info, gmok) : -1;
    if (ni < 1 || (int64_t)ni * K * L * M * 8 > 2 * SW_SCRATCH_MAX) {
        sw_free(o);
        rr_set_error("%s: F = %d, K = %d, nsamples = %d, minibatch = %d is outside the wide small-batch loop's range "
                     "(%s)", who, a.F, K, L, M, gmok ? "rr_glm_sviwgm_supported" : "rr_glm_sviw_supported");
        return RR_ERR_UNSUPPORTED;
    }
    std::vector<int> items((size_t)3 * ni);
    (void)sw_plan(n_children, pk, pn, pd, K, L, M, ni, items.data(), info, gmok);
    std::vector<SwItem> hitems((size_t)ni);
    for (int s = 0; s < n_children; ++s) o->hkid[s].item0 = -1;
    for (int i = 0; i < ni; ++i) {
        hitems[i].child = items[3 * i];
        hitems[i].j0 = items[3 * i + 1];
        hitems[i].cnt = items[3 * i + 2];
        SwChild &c = o->hkid[hitems[i].child];
        if (c.item0 < 0) c.item0 = i;
        c.nitems = i - c.item0 + 1;
    }
    a.nitems = ni;
    o->gm = gm_cols > 0;
    o->lds_bytes = (size_t)info[2];
    const size_t nb = (size_t)a.np * 8, nik = (size_t)ni * K;
    hipError_t e = rr_svi_state_alloc(o->st, a.np, maxiter, z0, lower, upper, is_log);
    if (e == hipSuccess) e = hipMalloc((void **)&o->dkid, sizeof(o->hkid));
    if (e == hipSuccess) e = hipMemcpy(o->dkid, o->hkid, sizeof(o->hkid), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&o->ditems, (size_t)ni * sizeof(SwItem));
    if (e == hipSuccess) e = hipMemcpy(o->ditems, hitems.data(), (size_t)ni * sizeof(SwItem), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMalloc((void **)&o->xbuf[0], nb);
    if (e == hipSuccess) e = hipMalloc((void **)&o->xbuf[1], nb);
    if (e == hipSuccess) e = hipMalloc((void **)&a.Phi, (size_t)M * a.F * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&a.fsp, nik * L * M * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&a.qp, nik * K * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&a.Rp, nik * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&a.dfs, (size_t)K * L * M * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&a.llp, (size_t)K * a.nbx * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&a.qf, (size_t)K * K * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&a.Rk, (size_t)n_children * K * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&a.n2p, nik * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&a.glsp, nik * maxls * 8);
    if (e == hipSuccess) e = hipMemset(a.glsp, 0, nik * maxls * 8);
    const void *dyn[2] = {o->gm ? (const void *)rr_glm_sviw_a_kernel<true> : (const void *)rr_glm_sviw_a_kernel<false>,
                          o->gm ? (const void *)rr_glm_sviw_c_kernel<true> : (const void *)rr_glm_sviw_c_kernel<false>};
    if (e == hipSuccess) e = hipFuncSetAttribute(dyn[0], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) e = hipFuncSetAttribute(dyn[1], hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e != hipSuccess) {
        (void)hipGetLastError();
        sw_free(o);
        rr_set_error("%s: %s", who, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? RR_ERR_OOM : RR_ERR_HIP;
    }
    const RrSviState &st = o->st;
    a.z = st.z; a.s1 = st.s1; a.s2 = st.s2; a.lower = st.lower; a.upper = st.upper; a.islog = st.islog; a.kid = o->dkid; a.items = o->ditems;
    sw_form_x(o);
    e = hipGetLastError();
    if (e != hipSuccess) {
        sw_free(o);
        rr_set_error("%s: %s", who, hipGetErrorString(e));
        return RR_ERR_HIP;
    }
    *out = o;
    return RR_OK;
}

int rr_glm_sviw_create(rr_ctx *ctx, int n_children, const rr_glm_sgd_child *children, const void *const *dX, const int *x_dtype,
                       const int64_t *ldx, int64_t N, const void *dy, const void *drowarg, const double *dlconst, int dtype, int K, int L,
                       int M, int lik, int n_lik, const double *z0, const double *lower, const double *upper, const unsigned char *is_log,
                       int updater, const double *upd_par, int64_t maxiter, double bmag, rr_glm_sviw **out) {
    return sw_create(false, ctx, n_children, children, dX, x_dtype, ldx, N, dy, drowarg, dlconst, dtype, K, L, M, lik, n_lik, z0, lower,
                     upper, is_log, updater, upd_par, maxiter, bmag, out);
}

int rr_glm_sviwgm_create(rr_ctx *ctx, int n_children, const rr_glm_sgd_child *children, const void *const *dX, const int *x_dtype,
                         const int64_t *ldx, int64_t N, const void *dy, const void *drowarg, const double *dlconst, int dtype, int K,
                         int L, int M, int lik, int n_lik, const double *z0, const double *lower, const double *upper,
                         const unsigned char *is_log, int updater, const double *upd_par, int64_t maxiter, double bmag,
                         rr_glm_sviw **out) {
    return sw_create(true, ctx, n_children, children, dX, x_dtype, ldx, N, dy, drowarg, dlconst, dtype, K, L, M, lik, n_lik, z0, lower,
                     upper, is_log, updater, upd_par, maxiter, bmag, out);
}

int rr_glm_sviw_set_start(rr_glm_sviw *o, const double *z0, const double *lower, const double *upper, const unsigned char *is_log) {
    RR_REQUIRE(o != nullptr && o->st.t == 0, "rr_glm_sviw_set_start: before the first step only");
    const int rc = rr_svi_state_set_start(o->st, o->ctx, z0, lower, upper, is_log);
    if (rc != RR_OK) return rc;
    sw_form_x(o);
    RR_CHECK_HIP(hipGetLastError());
    return RR_OK;
}

int rr_glm_sviw_run(rr_glm_sviw *o, int64_t steps, const int *d_idx, const float *dE, uint64_t seed, uint64_t key0) {
    RR_REQUIRE(o != nullptr && d_idx != nullptr && steps >= 1 && steps <= (1 << 20), "rr_glm_sviw_run: 1 <= steps <= 2^20 per call");
    RR_REQUIRE(o->st.t + steps <= o->st.maxiter, "rr_glm_sviw_run: %lld steps done, %lld more asked, %lld at most", (long long)o->st.t,
               (long long)steps, (long long)o->st.maxiter);
    rr_ctx *c = o->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    SwArgs a = o->a;
    const dim3 gi((unsigned)a.nitems, (unsigned)a.K), gb((unsigned)a.nbx, (unsigned)a.K), th(SW_THREADS);
    for (int64_t t = 0; t < steps; ++t) {
        const int64_t gt = o->st.t + t;
        a.idx = d_idx + (size_t)t * a.M;
        a.E = dE ? dE + (size_t)t * a.K * a.L * a.F : nullptr;
        // the key of rr_glm_draw_kernel for (seed, key0 + t); Adam's bias (sgd.py:322-323): nothing of either on the device
        a.stepkey = rr_svi_stepkey(seed, key0 + (uint64_t)t);
        rr_svi_adam_bias(a.up, gt + 1, a.b1t, a.b2t);
        a.xin = o->xbuf[gt & 1];
        a.xout = o->xbuf[(gt + 1) & 1];
        a.obj = o->st.objs + gt;
        a.norm = o->st.norms + gt;
        a.objective_only = 0;
        if (o->gm) {   // (the launch counters of the bounds build know an instance by the kernel's name alone)
            hipLaunchKernelGGL(rr_glm_sviw_a_kernel<true>, gi, th, o->lds_bytes, c->stream, a);
            hipLaunchKernelGGL(rr_glm_sviw_b_kernel, gb, th, 0, c->stream, a);
            hipLaunchKernelGGL(rr_glm_sviw_c_kernel<true>, gi, th, o->lds_bytes, c->stream, a);
            hipLaunchKernelGGL(rr_glm_sviw_d_kernel<true>, dim3(1), th, 0, c->stream, a);
        } else {
            hipLaunchKernelGGL(rr_glm_sviw_a_kernel<false>, gi, th, o->lds_bytes, c->stream, a);
            hipLaunchKernelGGL(rr_glm_sviw_b_kernel, gb, th, 0, c->stream, a);
            hipLaunchKernelGGL(rr_glm_sviw_c_kernel<false>, gi, th, o->lds_bytes, c->stream, a);
            hipLaunchKernelGGL(rr_glm_sviw_d_kernel<false>, dim3(1), th, 0, c->stream, a);
        }
    }
    RR_CHECK_HIP(hipGetLastError());
    o->st.t += steps;
    return RR_OK;
}

int rr_glm_sviw_starts(rr_glm_sviw *o, int ncand, const int *d_idx, const double *cand_host, const float *dE, uint64_t seed,
                       uint64_t key0, double *objs_host) {
    RR_REQUIRE(o != nullptr && d_idx != nullptr && cand_host != nullptr && objs_host != nullptr && ncand >= 1 && ncand < (1 << 20),
               "rr_glm_sviw_starts: bad argument");
    rr_ctx *c = o->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    SwArgs a = o->a;
    const int rc = rr_svi_state_candidates(o->st, c, ncand, cand_host);
    if (rc != RR_OK) return rc;
    const dim3 gi((unsigned)a.nitems, (unsigned)a.K), gb((unsigned)a.nbx, (unsigned)a.K), th(SW_THREADS);
    for (int s = 0; s < ncand; ++s) {
        a.idx = d_idx + (size_t)s * a.M;
        a.E = dE ? dE + (size_t)s * a.K * a.L * a.F : nullptr;
        a.stepkey = rr_svi_stepkey(seed, key0 + (uint64_t)s);
        a.xin = o->st.cand + (size_t)s * a.np;
        a.xout = nullptr;
        a.obj = o->st.out + s;
        a.norm = nullptr;
        a.objective_only = 1;
        if (o->gm) {
            hipLaunchKernelGGL(rr_glm_sviw_a_kernel<true>, gi, th, o->lds_bytes, c->stream, a);
            hipLaunchKernelGGL(rr_glm_sviw_b_kernel, gb, th, 0, c->stream, a);
            hipLaunchKernelGGL(rr_glm_sviw_d_kernel<true>, dim3(1), th, 0, c->stream, a);
        } else {
            hipLaunchKernelGGL(rr_glm_sviw_a_kernel<false>, gi, th, o->lds_bytes, c->stream, a);
            hipLaunchKernelGGL(rr_glm_sviw_b_kernel, gb, th, 0, c->stream, a);
            hipLaunchKernelGGL(rr_glm_sviw_d_kernel<false>, dim3(1), th, 0, c->stream, a);
        }
    }
    RR_CHECK_HIP(hipGetLastError());
    RR_CHECK_HIP(hipMemcpyAsync(objs_host, o->st.out, (size_t)ncand * 8, hipMemcpyDeviceToHost, c->stream));
    RR_CHECK_HIP(hipStreamSynchronize(c->stream));
    return RR_OK;
}

int rr_glm_sviw_read(rr_glm_sviw *o, double *z, double *objs, double *norms, int64_t *steps) {
    RR_REQUIRE(o != nullptr, "rr_glm_sviw_read: null argument");
    return rr_svi_state_read(o->st, o->ctx, z, objs, norms, steps);
}

void rr_glm_sviw_destroy(rr_glm_sviw *o) {
    if (!o) return;
    (void)hipSetDevice(o->ctx->device);
    (void)hipStreamSynchronize(o->ctx->stream);
    sw_free(o);
}

}  // extern "C"
