// =============================================================================================
// The GLM SVI step (glm.py:296-322) on the FLOAT64 feature matrix (rr_featmat64, rr_elbo.hip): GeneralizedLinearModel(dtype="f64").
//
//   WSt (ld, KLp), WSs = WSt^T / (K L)  weight samples ws = m_k + sqrt(C_k) e (or the caller's), zero padded   rr_glm64_ws_kernel
//   Pt = P^T                            the matrix' transposing pass                                             rr_transpose_f64_kernel
//   FS (rows_pad, KLp) = P WS^T         K = ld                                                                   rr_gemm_tn_f64_kernel
//   dfs = d loglike / d f, in place and transposed (DFSt); per-block partial sums of loglike                  rr_glm64_lik_kernel
//   llsum / aux per component           the partials added in a fixed order                                     rr_glm64_sum_kernel
//   Ed (KLp, ld) = dfs^T P              K = rows_pad, cut into row slabs when the tiles alone leave CUs idle    rr_gemm_tn_f64_kernel
//                                       (rr_glm64_plan), the slabs' partial tiles added in slab order           rr_glm64_slab_sum_kernel
//   EdPhi (rows_pad, ld) = dfs WSs      K = KLp (= dfs ws / (K L)), kept in the matrix' U for the children's contractions   rr_gemm_tn_f64_kernel
//   Edm, EdC (K, F)                     sums over the L samples of a component (glm.py:309-310)                  rr_glm64_reduce_kernel
//
// Padding is the float64 matrix': rows to 128 (rows_pad), F to ld, K L to a multiple of 128 (KLp); every padded element of an
// operand is WRITTEN as zero by the kernel that makes the operand.  The first product's operand WSt is not pre-scaled by
// 1 / (K L) (the f32 pipeline's guard against overflow of its products has no use in float64): f is the plain product P ws.
// Only WSs, the EdPhi product's operand, carries the 1 / (K L) of the mean over samples and components.
// No floating-point atomics anywhere in the step: the same bits every run, in either determinism mode (the one exception
// follows the library's convention: rr_glm_grad_t64_kernel adds its block partials atomically unless the context is
// deterministic, exactly like rr_grad_t64_kernel).
//
// The likelihood formulas below (glm64_lik) are the float64 master copy for the step-per-call pipeline; rr_svi_lik
// (rr_svi_common.h) is the small-minibatch loops' own (its softplus-link Poisson keeps the reference's clamp where this one is
// division-free).  tests/glm_f64_cases.py holds these
// to (16 + 4 |f|) 2^-53 S per element over -200 <= f <= 200.
// =============================================================================================
#include <algorithm>
#include <cstdlib>

#include "rr_internal.h"

int rr_launch_gemm_tn_f64(rr_ctx *c, const double *A, int64_t lda, const double *B, int64_t ldb, double *D, int64_t ldd,
                          int64_t K, int64_t M, int64_t N, int subtract, int upper_only);  // rr_rff.hip
int rr_launch_gemm_tn_f64_slabs(rr_ctx *c, const double *A, int64_t lda, const double *B, int64_t ldb, double *D, int64_t ldd,
                                int64_t K, int64_t M, int64_t N, int nslabs, int64_t kslab, int64_t slab_stride);  // rr_rff.hip
int rr_launch_transpose_f64(rr_ctx *c, const double *P, int64_t rows, int64_t ldp, double *Pt, int64_t ldt, int64_t cols_pad,
                            int64_t rows_pad);  // rr_elbo.hip

// ---- the one place that decides the Ed product's row slabs ----------------------------------------------------------------
// tiles = (KLp / 128) (ld / 128) output tiles, each with a k-loop of rows_pad.  One slab when the tiles alone are at least
// 2 num_cu; else the smallest count that brings tiles x slabs to num_cu, at most rows_pad / 128 -- moved up to the next count
// whose equal slab length (a multiple of 16) leaves the last slab non-empty (33 tiles of rows in 32 slabs of 144 would not).
// force > 0 (RR_GLM64_KSLABS) replaces the count before that adjustment.
static void glm64_plan(int64_t rows, int64_t F, int64_t KL, int num_cu, int force, int64_t out[4]) {
    const int64_t rp = (rows + 127) / 128 * 128, ld = (F + 127) / 128 * 128, klp = (KL + 127) / 128 * 128;
    const int64_t tiles = (klp / 128) * (ld / 128), q = rp / 128;
    if (num_cu < 1) num_cu = 1;
    int64_t s = 1;
    if (tiles < 2 * (int64_t)num_cu) s = ((int64_t)num_cu + tiles - 1) / tiles;
    if (force > 0) s = force;
    if (s > q) s = q;
    if (s < 1) s = 1;
    const int64_t r16 = rp / 16;
    while (s < q && (s - 1) * ((r16 + s - 1) / s) >= r16) ++s;
    out[0] = s;
    out[1] = 16 * ((r16 + s - 1) / s);
    out[2] = tiles;
    out[3] = rp;
}

// d loglike / d f and the f-dependent part of loglike (Gaussian: the squared error)   likelihoods.py:46-104,171-233,298-368,456-521
__device__ __forceinline__ void glm64_lik(int lik, double f, double y, double n, double ivar, double &df, double &ll) {
    if (lik == RR_LIK_GAUSSIAN) {
        const double er = y - f;
        df = er * ivar;
        ll = er * er;
        return;
    }
    if (lik == RR_LIK_POISSON_EXP) {
        const double g = exp(f);
        df = y - g;
        ll = y * f - g;
        return;
    }
    const double t = exp(-fabs(f));       // (0, 1]; 0 below |f| = 745
    const double u = 1.0 + t;
    const double l1p = log1p(t);          // softplus(f) = max(f, 0) + log1p(exp(-|f|))
    const bool pos = f >= 0.0;
    if (lik == RR_LIK_BERNOULLI || lik == RR_LIK_BINOMIAL) {
        const double nn = lik == RR_LIK_BINOMIAL ? n : 1.0;
        const double ex = pos ? 1.0 / u : t / u;   // the two-branch expit
        df = y - nn * ex;
        ll = y * f - nn * (fmax(f, 0.0) + l1p);
        return;
    }
    // Poisson, softplus link: g = softplus(f).  f >= 0: g >= log 2, the plain formulas.  f < 0: g = t q with q = log1p(t) / t in
    // [log 2, 1] underflows (and y / g overflows) long before the terms do, so expit(f) y / g is formed as y / ((1 + t) q) and
    // log g as f + log q: no division by g, nothing for the reference's max(g, 1e-100) to guard (rr_lik_elem, rr_elbo.hip)
    const double q = t > 0.0 ? l1p / t : 1.0;
    const double g = fmax(f, 0.0) + l1p;
    const double a = (pos ? 1.0 : t) / u;  // expit(f)
    const double b = y / (pos ? g : u * q);
    df = pos ? a * (b - 1.0) : b - a;
    ll = y * ((pos ? 0.0 : f) + log(pos ? g : q)) - g;
}

// WSs (klp, ld) = ws / (K L) and WSt (ld, klp) = ws^T from the caller's samples (DRAWS = false: src = WS (KL, F)) or from (m, C, E) (src = E (KL, F),
// component-major: k = kl / L; m, C (F, K)); 64 x 64 tiles through LDS, both stores coalesced; the padding is written as zeros
template <bool DRAWS>
__global__ void __launch_bounds__(256)
rr_glm64_ws_kernel(const double *__restrict__ src, const double *__restrict__ m, const double *__restrict__ C, int F, int K, int L,
                   int KL, int64_t ld, int64_t klp, double *__restrict__ WSs, double *__restrict__ WSt) {
    __shared__ double tile[64][65];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t f0 = (int64_t)blockIdx.x * 64, kl0 = (int64_t)blockIdx.y * 64;
    RR_DEV_ASSERT(f0 + 64 <= ld && kl0 + 64 <= klp);
#pragma unroll
    for (int k = 0; k < 16; ++k) {
        const int64_t kl = kl0 + ty + 4 * k, f = f0 + tx;
        double w = 0.0;
        if (kl < KL && f < F) {
            const double e = src[kl * F + f];
            if (DRAWS) {
                const int64_t o = f * K + kl / L;
                w = m[o] + sqrt(C[o]) * e;
            } else {
                w = e;
            }
        }
        WSs[kl * ld + f] = w / (double)KL;   // EdPhi's operand: glm.py:315's mean over the L samples and K components
        tile[ty + 4 * k][tx] = w;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 16; ++k) WSt[(f0 + ty + 4 * k) * klp + kl0 + tx] = tile[tx][ty + 4 * k];
}

// FS (rows_pad, ldf) -> dfs in place and DFSt (ldf, ldt) = dfs^T (STORE; rows >= `rows` and samples >= KL as zeros), and the
// block's sum of the log-likelihood terms per sample into part[blockIdx.y][kl]: thread (tx, ty) adds its 16 rows in row order,
// the four ty of a sample are added in ty order -- a fixed order, no atomics.  64 samples x 64 rows per block.
template <typename TY, bool STORE>
__global__ void __launch_bounds__(256)
rr_glm64_lik_kernel(double *__restrict__ FS, int64_t rows, int64_t rows_pad, int64_t ldf, const TY *__restrict__ y,
                    const TY *__restrict__ rowarg, int lik, double ivar, int KL, double *__restrict__ DFSt, int64_t ldt,
                    double *__restrict__ part) {
    __shared__ double tile[64][65];
    __shared__ double psum[4][64];
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const int64_t kl0 = (int64_t)blockIdx.x * 64, r0 = (int64_t)blockIdx.y * 64;
    const int64_t kl = kl0 + tx;
    RR_DEV_ASSERT(kl0 + 64 <= ldf && r0 + 64 <= rows_pad && rows_pad <= ldt);
    double acc = 0.0;
#pragma unroll 4
    for (int k = 0; k < 16; ++k) {
        const int64_t r = r0 + ty + 4 * k;
        double df = 0.0;
        if (kl < KL && r < rows) {
            double ll;
            glm64_lik(lik, FS[r * ldf + kl], (double)y[r], lik == RR_LIK_BINOMIAL ? (double)rowarg[r] : 0.0, ivar, df, ll);
            acc += ll;
        }
        if (STORE) {
            FS[r * ldf + kl] = df;
            tile[ty + 4 * k][tx] = df;
        }
    }
    psum[ty][tx] = acc;
    __syncthreads();
    if (STORE) {
#pragma unroll
        for (int k = 0; k < 16; ++k) DFSt[(kl0 + ty + 4 * k) * ldt + r0 + tx] = tile[tx][ty + 4 * k];
    }
    if (ty == 0) part[(int64_t)blockIdx.y * ldf + kl] = ((psum[0][tx] + psum[1][tx]) + psum[2][tx]) + psum[3][tx];
}

// llsum[k] / aux[k] from the likelihood kernel's partials (nrt row tiles x ldf samples): thread t of block k adds the samples
// l = t, t + 256, .. of component k, each over the row tiles in tile order; thread 0 adds the 256 thread sums in thread order
__global__ void __launch_bounds__(256)
rr_glm64_sum_kernel(const double *__restrict__ part, int64_t nrt, int64_t ldf, int L, int lik, double ivar,
                    double *__restrict__ llsum, double *__restrict__ aux) {
    __shared__ double red[256];
    const int k = blockIdx.x, t = threadIdx.x;
    double s = 0.0;
    for (int l = t; l < L; l += 256) {
        const int64_t c = (int64_t)k * L + l;
        RR_DEV_ASSERT(c < ldf);
        for (int64_t rt = 0; rt < nrt; ++rt) s += part[rt * ldf + c];
    }
    red[t] = s;
    __syncthreads();
    if (t == 0) {
        double tot = 0.0;
        const int nt = L < 256 ? L : 256;
        for (int i = 0; i < nt; ++i) tot += red[i];
        if (lik == RR_LIK_GAUSSIAN) {
            aux[k] = tot;
            llsum[k] = -0.5 * tot * ivar;
        } else {
            aux[k] = 0.0;
            llsum[k] = tot;
        }
    }
}

// Ed[i] = sum_s part[s * stride + i] in slab order (the Ed product's row slabs)
__global__ void __launch_bounds__(256)
rr_glm64_slab_sum_kernel(const double *__restrict__ part, int nslabs, int64_t stride, int64_t count, double *__restrict__ Ed) {
    const int64_t i = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 2;
    if (i >= count) return;
    RR_DEV_ASSERT(i + 2 <= count && count <= stride);
    double2 a = *reinterpret_cast<const double2 *>(part + i);
    for (int s = 1; s < nslabs; ++s) {
        const double2 b = *reinterpret_cast<const double2 *>(part + (int64_t)s * stride + i);
        a.x += b.x;
        a.y += b.y;
    }
    *reinterpret_cast<double2 *>(Ed + i) = a;
}

// Edm[k][f] = sum_l Ed[kL + l][f] / L;   EdC[k][f] = sum_l Ed[kL + l][f] e[kL + l][f] / (L sqrt(C[f][k]))   (glm.py:309-310)
__global__ void __launch_bounds__(256)
rr_glm64_reduce_kernel(const double *__restrict__ Ed, const double *__restrict__ E, const double *__restrict__ C, int F, int K,
                       int L, int64_t ld, double *__restrict__ Edm, double *__restrict__ EdC) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)K * F) return;
    const int k = (int)(i / F), f = (int)(i % F);
    RR_DEV_ASSERT(f < ld);
    double a = 0.0, b = 0.0;
    for (int l = 0; l < L; ++l) {
        const int64_t kl = (int64_t)k * L + l;
        const double ed = Ed[kl * ld + f];
        a += ed;
        b += ed * E[kl * F + f];
    }
    Edm[i] = a / L;
    EdC[i] = b / (L * sqrt(C[(int64_t)f * K + k]));
}

// T[i][f] += sum_r x[r][i] (E[r][n + f] P[r][f] - E[r][f] P[r][n + f]): rr_glm_grad_t_kernel in float64 (E = EdPhi, the matrix'
// U); block partials through rr_acc_out, as rr_grad_t64_kernel
template <int DMAX, typename TX>
__global__ void __launch_bounds__(256)
rr_glm_grad_t64_kernel(const TX *__restrict__ X, int64_t N, int64_t ldx, const double *__restrict__ P, const double *__restrict__ E,
                       int64_t ldp, int n, int d, double *__restrict__ T, int rows_per_block, int64_t tdet) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    const bool fvalid = f < n;
    const int fc = fvalid ? f : 0;
    RR_DEV_ASSERT(DMAX <= ldx && d <= DMAX);
    double t[DMAX];
#pragma unroll
    for (int i = 0; i < DMAX; ++i) t[i] = 0.0;
    const int64_t r0 = (int64_t)blockIdx.y * rows_per_block;
    int64_t r1 = r0 + rows_per_block;
    if (r1 > N) r1 = N;
    for (int64_t r = r0; r < r1; ++r) {
        const double a = E[r * ldp + n + fc] * P[r * ldp + fc] - E[r * ldp + fc] * P[r * ldp + n + fc];
        const TX *xr = X + r * ldx;
#pragma unroll
        for (int i = 0; i < DMAX; ++i) t[i] = fma((double)xr[i], a, t[i]);
    }
    if (fvalid) {
#pragma unroll
        for (int i = 0; i < DMAX; ++i)
            if (i < d) rr_acc_out(T, tdet, blockIdx.y, (int64_t)i * n + f, t[i]);
    }
}

// ---- the wide contraction T = X^T A (rr_featmat64_pass2_xt / rr_featmat64_glm_xt, 128 < Xdim <= 4096) ----------------------------
// A one-frequency-per-thread VALU kernel holds Xdim accumulators in registers; above 128 columns the 2 rows d n flops go to the
// float64 matrix cores instead: A (rows_pad, npad) is formed once in the matrix' Pt scratch (free once U holds Phi C or EdPhi),
// X is staged as float64 (rows_pad, wp) panels of at most wp columns, rr_gemm_tn_f64_kernel contracts them over its row slabs
// (glm64_plan's rule: tiles = (wp / 128)(npad / 128)) and the slabs' tiles are added into T in slab order.  npad, wp: multiples
// of 128; every padded element of both operands is written as zero.  No atomics: the same bits every run.

// A[r][f] for the trig block pair (P, U point at the pair's first column; 2 n <= ldp - col0).  GLM: E_s P_c - E_c P_s against
// the stored EdPhi (U); else err (P_c m_s - P_s m_c) - (P_c U_s - P_s U_c), the operand of rr_grad_t64_kernel.  A wave writes
// 64 double2 = one 1 KiB run of a row; 4 rows per block pass, blocks stride over the rows.
template <bool GLM>
__global__ void __launch_bounds__(256)
rr_fm64_form_a_kernel(const double *__restrict__ P, const double *__restrict__ U, int64_t ldp, int64_t col0,
                      const double *__restrict__ err, const double *__restrict__ mvec, int64_t rows, int64_t rows_pad, int n,
                      int64_t npad, double *__restrict__ A) {
    const int f = 2 * (blockIdx.x * 64 + (threadIdx.x & 63));
    RR_DEV_ASSERT(f + 2 <= npad && n <= npad && col0 + 2 * (int64_t)n <= ldp && rows <= rows_pad);
    const bool v0 = f < n, v1 = f + 1 < n;
    const int f0 = v0 ? f : 0, f1 = v1 ? f + 1 : 0;
    double mc0 = 0.0, mc1 = 0.0, ms0 = 0.0, ms1 = 0.0;
    if (!GLM) {
        mc0 = mvec[f0];
        mc1 = mvec[f1];
        ms0 = mvec[n + f0];
        ms1 = mvec[n + f1];
    }
    for (int64_t r = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6); r < rows_pad; r += (int64_t)gridDim.y * 4) {
        double2 a;
        a.x = 0.0;
        a.y = 0.0;
        if (r < rows) {
            const double *p = P + r * ldp, *u = U + r * ldp;
            const double pc0 = p[f0], pc1 = p[f1], ps0 = p[n + f0], ps1 = p[n + f1];
            const double uc0 = u[f0], uc1 = u[f1], us0 = u[n + f0], us1 = u[n + f1];
            if (GLM) {
                a.x = us0 * pc0 - uc0 * ps0;
                a.y = us1 * pc1 - uc1 * ps1;
            } else {
                const double e = err[r];
                a.x = e * (pc0 * ms0 - ps0 * mc0) - (pc0 * us0 - ps0 * uc0);
                a.y = e * (pc1 * ms1 - ps1 * mc1) - (pc1 * us1 - ps1 * uc1);
            }
            if (!v0) a.x = 0.0;
            if (!v1) a.y = 0.0;
        }
        *reinterpret_cast<double2 *>(A + r * npad + f) = a;
    }
}

// Xs (rows_pad, wp) = the columns [i0, i0 + w) of X (rows, ldx) as float64, zero beyond w and beyond `rows`
template <typename TX>
__global__ void __launch_bounds__(256)
rr_fm64_stage_x_kernel(const TX *__restrict__ X, int64_t rows, int64_t rows_pad, int64_t ldx, int i0, int w, int64_t wp,
                       double *__restrict__ Xs) {
    const int c = 2 * (blockIdx.x * 64 + (threadIdx.x & 63));
    RR_DEV_ASSERT(c + 2 <= wp && w <= wp && i0 + w <= ldx && rows <= rows_pad);
    for (int64_t r = (int64_t)blockIdx.y * 4 + (threadIdx.x >> 6); r < rows_pad; r += (int64_t)gridDim.y * 4) {
        double2 v;
        v.x = 0.0;
        v.y = 0.0;
        if (r < rows) {
            const TX *x = X + r * ldx + i0;
            if (c < w) v.x = (double)x[c];
            if (c + 1 < w) v.y = (double)x[c + 1];
        }
        *reinterpret_cast<double2 *>(Xs + r * wp + c) = v;
    }
}

// T[(i0 + i) n + f] += sum_s part[s stride + i npad + f] in slab order, i < w, f < n
__global__ void __launch_bounds__(256)
rr_fm64_xt_sum_kernel(const double *__restrict__ part, int nslabs, int64_t stride, int64_t npad, int n, int i0, int w,
                      double *__restrict__ T) {
    const int f = blockIdx.x * 256 + threadIdx.x;
    const int i = blockIdx.y;
    if (f >= n) return;
    RR_DEV_ASSERT(i < w && n <= npad && (int64_t)w * npad <= stride);
    double a = part[(int64_t)i * npad + f];
    for (int s = 1; s < nslabs; ++s) a += part[(int64_t)s * stride + (int64_t)i * npad + f];
    T[(int64_t)(i0 + i) * n + f] += a;
}

int rr_fm64_xt_wide(rr_featmat64 *fm, bool glm, const void *dX, int x_dtype, int64_t ldx, int d, int n, int64_t col0, double *dT) {
    rr_ctx *c = fm->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    const int64_t rp = fm->rows_pad, npad = ((int64_t)n + 127) / 128 * 128, dp = ((int64_t)d + 127) / 128 * 128;
    RR_REQUIRE(fm->Pt != nullptr && npad <= fm->ld && rp <= fm->max_rows, "float64 feature matrix: no room for the contraction's operand");
    // X panels of at most 2^27 staged elements (1 GiB)
    int64_t wp = ((int64_t)1 << 27) / rp / 128 * 128;
    if (wp < 128) wp = 128;
    if (wp > dp) wp = dp;
    const char *fs = getenv("RR_GLM64_KSLABS");  // measurement switch: force the slab count (as the step's Ed product)
    const int force = fs ? atoi(fs) : 0;
    size_t need = 0;
    for (int64_t i0 = 0; i0 < d; i0 += wp) {
        const int64_t w = std::min<int64_t>(wp, d - i0), w128 = (w + 127) / 128 * 128;
        int64_t plan[4];
        glm64_plan(fm->rows, n, w128, c->num_cu, force, plan);
        need = std::max(need, (size_t)(rp * w128 + plan[0] * w128 * npad));
    }
    if (fm->xt_elems < need) {
        RR_CHECK_HIP(hipStreamSynchronize(c->stream));
        if (fm->xt) (void)hipFree(fm->xt);
        fm->xt = nullptr;
        fm->xt_elems = 0;
        if (hipMalloc((void **)&fm->xt, need * 8) != hipSuccess) {
            (void)hipGetLastError();
            rr_set_error("float64 feature matrix: device allocation of the wide contraction's scratch (%zu bytes) failed", need * 8);
            return RR_ERR_OOM;
        }
        fm->xt_elems = need;
    }
    double *A = fm->Pt;
    const unsigned gy = (unsigned)std::min<int64_t>((rp + 3) / 4, 65535);
    if (glm)
        hipLaunchKernelGGL(rr_fm64_form_a_kernel<true>, dim3((unsigned)(npad / 128), gy), dim3(256), 0, c->stream, fm->P + col0,
                           fm->U + col0, fm->ld, col0, (const double *)nullptr, (const double *)nullptr, fm->rows, rp, n, npad, A);
    else
        hipLaunchKernelGGL(rr_fm64_form_a_kernel<false>, dim3((unsigned)(npad / 128), gy), dim3(256), 0, c->stream, fm->P + col0,
                           fm->U + col0, fm->ld, col0, fm->err, fm->m + col0, fm->rows, rp, n, npad, A);
    RR_CHECK_HIP(hipGetLastError());
    for (int64_t i0 = 0; i0 < d; i0 += wp) {
        const int64_t w = std::min<int64_t>(wp, d - i0), w128 = (w + 127) / 128 * 128;
        double *Xs = fm->xt, *part = fm->xt + rp * w128;
        if (x_dtype == RR_F32)
            hipLaunchKernelGGL(rr_fm64_stage_x_kernel<float>, dim3((unsigned)(w128 / 128), gy), dim3(256), 0, c->stream, (const float *)dX,
                               fm->rows, rp, ldx, (int)i0, (int)w, w128, Xs);
        else
            hipLaunchKernelGGL(rr_fm64_stage_x_kernel<double>, dim3((unsigned)(w128 / 128), gy), dim3(256), 0, c->stream, (const double *)dX,
                               fm->rows, rp, ldx, (int)i0, (int)w, w128, Xs);
        RR_CHECK_HIP(hipGetLastError());
        int64_t plan[4];
        glm64_plan(fm->rows, n, w128, c->num_cu, force, plan);
        const int64_t stride = w128 * npad;
        int rc = rr_launch_gemm_tn_f64_slabs(c, Xs, w128, A, npad, part, npad, rp, w128, npad, (int)plan[0], plan[1], stride);
        if (rc != RR_OK) return rc;
        hipLaunchKernelGGL(rr_fm64_xt_sum_kernel, dim3((unsigned)((n + 255) / 256), (unsigned)w), dim3(256), 0, c->stream, part,
                           (int)plan[0], stride, npad, n, (int)i0, (int)w, dT);
        RR_CHECK_HIP(hipGetLastError());
    }
    return RR_OK;
}

// ---- scratch: next to the matrix' second-pass scratch (rr_featmat64::glm), allocated by the first step, grown when K L grows ----
struct Glm64Scratch {
    double *WSs = nullptr, *WSt = nullptr, *FS = nullptr, *DFSt = nullptr, *Ed = nullptr, *Eraw = nullptr, *part = nullptr;
    double *mc = nullptr;    // [m (F K) | C (F K) | Edm (K F) | EdC (K F)]
    double *kacc = nullptr;  // [llsum (kcap) | aux (kcap)]
    double *edpart = nullptr;  // the Ed product's slabs, grow-only
    size_t edpart_elems = 0;
    int64_t klp = 0;
    int kcap = 0;
};

static void glm64_free(Glm64Scratch *s) {
    void *q[] = {s->WSs, s->WSt, s->FS, s->DFSt, s->Ed, s->Eraw, s->part, s->mc, s->kacc, s->edpart};
    for (void *x : q)
        if (x) (void)hipFree(x);
    *s = Glm64Scratch();
}

void rr_glm64_scratch_free(void *p) {
    if (!p) return;
    glm64_free((Glm64Scratch *)p);
    delete (Glm64Scratch *)p;
}

static int glm64_scratch(rr_featmat64 *fm, int64_t klp, int K) {
    int rc = rr_fm64_scratch(fm);
    if (rc != RR_OK) return rc;
    if (!fm->glm) fm->glm = new Glm64Scratch();
    Glm64Scratch &s = *(Glm64Scratch *)fm->glm;
    if (s.klp >= klp && s.kcap >= K) return RR_OK;
    RR_CHECK_HIP(hipStreamSynchronize(fm->ctx->stream));
    if (klp < s.klp) klp = s.klp;
    if (K < s.kcap) K = s.kcap;
    glm64_free(&s);
    const size_t ld = (size_t)fm->ld, mr = (size_t)fm->max_rows, kl = (size_t)klp;
    hipError_t e = hipMalloc((void **)&s.WSs, kl * ld * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&s.WSt, ld * kl * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&s.FS, mr * kl * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&s.DFSt, kl * mr * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&s.Ed, kl * ld * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&s.Eraw, kl * ld * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&s.part, (mr / 64) * kl * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&s.mc, (size_t)4 * fm->F * K * 8);
    if (e == hipSuccess) e = hipMalloc((void **)&s.kacc, (size_t)2 * K * 8);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        glm64_free(&s);
        rr_set_error("float64 feature matrix: device allocation of the GLM step's scratch failed");
        return RR_ERR_OOM;
    }
    s.klp = klp;
    s.kcap = K;
    return RR_OK;
}

static int glm64_checks(rr_featmat64 *fm, const void *dy, const void *drowarg, int dtype, int lik, double lik_param, int K, int L,
                        const char *who) {
    RR_REQUIRE(fm != nullptr && dy != nullptr, "%s: null argument", who);
    RR_REQUIRE(fm->rows == 0 || fm->covered == fm->F, "%s: only %lld of the %d columns were written since rr_featmat64_begin", who,
               (long long)fm->covered, fm->F);
    RR_REQUIRE(dtype == RR_F32 || dtype == RR_F64, "%s: bad dtype", who);
    RR_REQUIRE(lik >= RR_LIK_BERNOULLI && lik <= RR_LIK_POISSON_SOFTPLUS, "%s: unknown likelihood %d", who, lik);
    RR_REQUIRE(lik != RR_LIK_BINOMIAL || drowarg != nullptr, "%s: the binomial needs its per-row n", who);
    RR_REQUIRE(lik != RR_LIK_GAUSSIAN || lik_param > 0.0, "%s: the Gaussian variance must be > 0", who);
    RR_REQUIRE(K >= 1 && L >= 1 && (int64_t)K * L < (1 << 24), "%s: bad K, L", who);
    RR_REQUIRE(fm->rows >= 1, "%s: the feature matrix is empty", who);
    return RR_OK;
}

// With WSs / WSt on the device: fs, the likelihood derivatives and sums, and -- unless objective_only -- Ed and EdPhi
static int glm64_pipeline(rr_featmat64 *fm, Glm64Scratch &s, const void *dy, const void *drowarg, int dtype, int lik,
                          double lik_param, int K, int L, bool objective_only) {
    rr_ctx *c = fm->ctx;
    const int KL = K * L;
    const int64_t ld = fm->ld, klp = s.klp, rp = fm->rows_pad;
    int rc = rr_launch_transpose_f64(c, fm->P, fm->rows, ld, fm->Pt, fm->max_rows, ld, rp);
    if (rc != RR_OK) return rc;
    rc = rr_launch_gemm_tn_f64(c, fm->Pt, fm->max_rows, s.WSt, klp, s.FS, klp, ld, rp, klp, 0, 0);
    if (rc != RR_OK) return rc;
    const double ivar = lik == RR_LIK_GAUSSIAN ? 1.0 / lik_param : 0.0;
    const dim3 lg((unsigned)(klp / 64), (unsigned)(rp / 64));
#define RR_GL64(TY, ST)                                                                                                        \
    hipLaunchKernelGGL((rr_glm64_lik_kernel<TY, ST>), lg, dim3(256), 0, c->stream, s.FS, fm->rows, rp, klp, (const TY *)dy, \
                       (const TY *)drowarg, lik, ivar, KL, s.DFSt, fm->max_rows, s.part)
    if (dtype == RR_F32) {
        if (objective_only) RR_GL64(float, false);
        else RR_GL64(float, true);
    } else {
        if (objective_only) RR_GL64(double, false);
        else RR_GL64(double, true);
    }
#undef RR_GL64
    hipLaunchKernelGGL(rr_glm64_sum_kernel, dim3((unsigned)K), dim3(256), 0, c->stream, s.part, rp / 64, klp, L, lik, ivar, s.kacc,
                       s.kacc + s.kcap);
    RR_CHECK_HIP(hipGetLastError());
    if (objective_only) return RR_OK;
    // Ed (klp, ld) = dfs^T P over the rows, in row slabs where the output tiles alone would leave compute units idle
    const char *fs = getenv("RR_GLM64_KSLABS");  // measurement switch: force the slab count
    int64_t plan[4];
    glm64_plan(fm->rows, fm->F, KL, c->num_cu, fs ? atoi(fs) : 0, plan);
    const int nslabs = (int)plan[0];
    if (nslabs == 1) {
        rc = rr_launch_gemm_tn_f64(c, s.FS, klp, fm->P, ld, s.Ed, ld, rp, klp, ld, 0, 0);
        if (rc != RR_OK) return rc;
    } else {
        const size_t stride = (size_t)klp * ld, need = stride * nslabs;
        if (s.edpart_elems < need) {
            RR_CHECK_HIP(hipStreamSynchronize(c->stream));
            if (s.edpart) (void)hipFree(s.edpart);
            s.edpart = nullptr;
            s.edpart_elems = 0;
            RR_CHECK_HIP(hipMalloc((void **)&s.edpart, need * 8));
            s.edpart_elems = need;
        }
        rc = rr_launch_gemm_tn_f64_slabs(c, s.FS, klp, fm->P, ld, s.edpart, ld, rp, klp, ld, nslabs, plan[1], (int64_t)stride);
        if (rc != RR_OK) return rc;
        hipLaunchKernelGGL(rr_glm64_slab_sum_kernel, dim3((unsigned)((stride / 2 + 255) / 256)), dim3(256), 0, c->stream, s.edpart,
                           nslabs, (int64_t)stride, (int64_t)stride, s.Ed);
        RR_CHECK_HIP(hipGetLastError());
    }
    // EdPhi (rows_pad, ld) = dfs WSs, kept in U for the children's gradient contractions
    rc = rr_launch_gemm_tn_f64(c, s.DFSt, fm->max_rows, s.WSs, ld, fm->U, ld, klp, rp, ld, 0, 0);
    if (rc != RR_OK) return rc;
    fm->have_edphi = true;
    return RR_OK;
}

// host (KL, F) float64 -> Eraw, then the weight-sample kernel
static int glm64_weights(rr_featmat64 *fm, Glm64Scratch &s, const double *src, bool draws, int K, int L) {
    rr_ctx *c = fm->ctx;
    const int KL = K * L, F = fm->F;
    RR_CHECK_HIP(hipMemcpyAsync(s.Eraw, src, (size_t)KL * F * 8, hipMemcpyHostToDevice, c->stream));
    const size_t fk = (size_t)F * K;
    const dim3 grid((unsigned)(fm->ld / 64), (unsigned)(s.klp / 64));
    if (draws)
        hipLaunchKernelGGL(rr_glm64_ws_kernel<true>, grid, dim3(256), 0, c->stream, s.Eraw, s.mc, s.mc + fk, F, K, L, KL, fm->ld, s.klp,
                           s.WSs, s.WSt);
    else
        hipLaunchKernelGGL(rr_glm64_ws_kernel<false>, grid, dim3(256), 0, c->stream, s.Eraw, (const double *)nullptr,
                           (const double *)nullptr, F, K, L, KL, fm->ld, s.klp, s.WSs, s.WSt);
    RR_CHECK_HIP(hipGetLastError());
    return RR_OK;
}

// rr_glm_grad_t64_kernel over the rows of the last step for the trig block pair at [col0, col0 + 2n): dT (d, n) += X^T A against
// EdPhi (d <= dpad <= 128, ldx >= dpad); block partials by atomics, or -- deterministic -- added in block order
static int glm64_grad_t(rr_featmat64 *fm, const void *dX, int x_dtype, int64_t ldx, int d, int dpad, int n, int64_t col0, double *dT) {
    rr_ctx *c = fm->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    const int64_t N = fm->rows;
    const int fblocks = (n + 255) / 256;
    int64_t rpb = (N * fblocks + (int64_t)c->num_cu * 8 - 1) / ((int64_t)c->num_cu * 8);
    if (rpb < 64) rpb = 64;
    if ((N + rpb - 1) / rpb > 65535) rpb = (N + 65534) / 65535;
    const dim3 grid(fblocks, (unsigned)((N + rpb - 1) / rpb));
    const int64_t tcount = (int64_t)d * n, tdet = c->deterministic ? tcount : 0;
    double *Tdst = dT;
    if (tdet) {
        void *part = nullptr;
        int rc = rr_det_scratch(c, (size_t)grid.y * (size_t)tcount * 8, &part);
        if (rc != RR_OK) return rc;
        Tdst = (double *)part;
    }
#define RR_GG64(DM, TX)                                                                                                          \
    hipLaunchKernelGGL((rr_glm_grad_t64_kernel<DM, TX>), grid, dim3(256), 0, c->stream, (const TX *)dX, N, ldx, fm->P + col0,    \
                       fm->U + col0, fm->ld, n, d, Tdst, (int)rpb, tdet)
#define RR_GG64D(DM)                           \
    if (x_dtype == RR_F32) RR_GG64(DM, float); \
    else RR_GG64(DM, double)
    switch (dpad) {
        case 8: RR_GG64D(8); break;
        case 16: RR_GG64D(16); break;
        case 32: RR_GG64D(32); break;
        case 64: RR_GG64D(64); break;
        default: RR_GG64D(128); break;
    }
#undef RR_GG64D
#undef RR_GG64
    RR_CHECK_HIP(hipGetLastError());
    return tdet ? rr_det_reduce(c, Tdst, grid.y, tcount, tcount, dT) : RR_OK;
}

extern "C" {

int rr_glm64_plan(int64_t rows, int64_t F, int KL, int num_cu, int64_t out[4]) {
    RR_REQUIRE(out != nullptr && rows >= 1 && F >= 1 && KL >= 1, "rr_glm64_plan: bad argument");
    glm64_plan(rows, F, KL, num_cu, 0, out);
    return RR_OK;
}

int rr_featmat64_glm_step(rr_featmat64 *fm, const void *dy, const void *drowarg, int dtype, int lik, double lik_param,
                          const double *WS, int K, int L, double *Edws, double *llsum, double *aux) {
    int rc = glm64_checks(fm, dy, drowarg, dtype, lik, lik_param, K, L, "rr_featmat64_glm_step");
    if (rc != RR_OK) return rc;
    RR_REQUIRE(WS != nullptr && Edws != nullptr && llsum != nullptr && aux != nullptr, "rr_featmat64_glm_step: null argument");
    rr_ctx *c = fm->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    const int KL = K * L, F = fm->F;
    rc = glm64_scratch(fm, ((int64_t)KL + 127) / 128 * 128, K);
    if (rc != RR_OK) return rc;
    Glm64Scratch &s = *(Glm64Scratch *)fm->glm;
    fm->have_rows = false;   // Pt and U are this step's from here on
    fm->have_edphi = false;
    rc = glm64_weights(fm, s, WS, false, K, L);
    if (rc == RR_OK) rc = glm64_pipeline(fm, s, dy, drowarg, dtype, lik, lik_param, K, L, false);
    if (rc != RR_OK) return rc;
    std::vector<double> acc((size_t)2 * s.kcap);
    RR_CHECK_HIP(hipMemcpy2DAsync(Edws, (size_t)F * 8, s.Ed, (size_t)fm->ld * 8, (size_t)F * 8, (size_t)KL, hipMemcpyDeviceToHost,
                                  c->stream));
    RR_CHECK_HIP(hipMemcpyAsync(acc.data(), s.kacc, acc.size() * 8, hipMemcpyDeviceToHost, c->stream));
    RR_CHECK_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < K; ++k) {
        llsum[k] = acc[k];
        aux[k] = acc[s.kcap + k];
    }
    return RR_OK;
}

int rr_featmat64_glm_step_draws(rr_featmat64 *fm, const void *dy, const void *drowarg, int dtype, int lik, double lik_param,
                                const double *m, const double *C, int K, int L, const double *E, double *Edm, double *EdC,
                                double *llsum, double *aux) {
    int rc = glm64_checks(fm, dy, drowarg, dtype, lik, lik_param, K, L, "rr_featmat64_glm_step_draws");
    if (rc != RR_OK) return rc;
    const bool objective_only = (Edm == nullptr && EdC == nullptr);  // llsum / aux only (random starts)
    RR_REQUIRE(m != nullptr && C != nullptr && E != nullptr && (objective_only || (Edm != nullptr && EdC != nullptr)) &&
               llsum != nullptr && aux != nullptr, "rr_featmat64_glm_step_draws: null argument");
    rr_ctx *c = fm->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    const int KL = K * L, F = fm->F;
    rc = glm64_scratch(fm, ((int64_t)KL + 127) / 128 * 128, K);
    if (rc != RR_OK) return rc;
    Glm64Scratch &s = *(Glm64Scratch *)fm->glm;
    fm->have_rows = false;
    fm->have_edphi = false;
    const size_t fk = (size_t)F * K;
    RR_CHECK_HIP(hipMemcpyAsync(s.mc, m, fk * 8, hipMemcpyHostToDevice, c->stream));
    RR_CHECK_HIP(hipMemcpyAsync(s.mc + fk, C, fk * 8, hipMemcpyHostToDevice, c->stream));
    rc = glm64_weights(fm, s, E, true, K, L);
    if (rc == RR_OK) rc = glm64_pipeline(fm, s, dy, drowarg, dtype, lik, lik_param, K, L, objective_only);
    if (rc != RR_OK) return rc;
    std::vector<double> acc((size_t)2 * s.kcap);
    if (!objective_only) {
        hipLaunchKernelGGL(rr_glm64_reduce_kernel, dim3((unsigned)((fk + 255) / 256)), dim3(256), 0, c->stream, s.Ed, s.Eraw, s.mc + fk, F,
                           K, L, fm->ld, s.mc + 2 * fk, s.mc + 3 * fk);
        RR_CHECK_HIP(hipGetLastError());
        RR_CHECK_HIP(hipMemcpyAsync(Edm, s.mc + 2 * fk, fk * 8, hipMemcpyDeviceToHost, c->stream));
        RR_CHECK_HIP(hipMemcpyAsync(EdC, s.mc + 3 * fk, fk * 8, hipMemcpyDeviceToHost, c->stream));
    }
    RR_CHECK_HIP(hipMemcpyAsync(acc.data(), s.kacc, acc.size() * 8, hipMemcpyDeviceToHost, c->stream));
    RR_CHECK_HIP(hipStreamSynchronize(c->stream));
    for (int k = 0; k < K; ++k) {
        llsum[k] = acc[k];
        aux[k] = acc[s.kcap + k];
    }
    return RR_OK;
}

int rr_featmat64_glm_rff(rr_featmat64 *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, int64_t col0, double *dT) {
    RR_REQUIRE(fm != nullptr && fm->U != nullptr && fm->have_edphi, "rr_featmat64_glm_rff: call rr_featmat64_glm_step first");
    RR_REQUIRE(b != nullptr && b->kind == RR_KIND_RFF && dT != nullptr && dX != nullptr, "rr_featmat64_glm_rff: bad argument");
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "rr_featmat64_glm_rff: bad dtype");
    RR_REQUIRE(col0 >= 0 && col0 + 2 * (int64_t)b->n <= fm->F, "rr_featmat64_glm_rff: columns out of range");
    RR_REQUIRE(ldx >= b->dpad && !b->large, "rr_featmat64_glm_rff: device X needs ldx >= rr_rff_padded_dim() = %d, Xdim <= 128", b->dpad);
    return glm64_grad_t(fm, dX, x_dtype, ldx, b->d, b->dpad, b->n, col0, dT);
}

// The same contraction against EdPhi for any trig block pair at [col0, col0 + 2n) and rows of 1 <= d <= 4096 columns, without a
// random Fourier handle (rr_featmat64_pass2_xt's twin: the register kernel up to 128 columns, the float64 GEMM above)
int rr_featmat64_glm_xt(rr_featmat64 *fm, const void *dX, int x_dtype, int64_t ldx, int d, int n, int64_t col0, double *dT) {
    RR_REQUIRE(fm != nullptr && fm->U != nullptr && fm->have_edphi, "rr_featmat64_glm_xt: call rr_featmat64_glm_step first");
    RR_REQUIRE(dT != nullptr && n >= 1, "rr_featmat64_glm_xt: bad argument");
    RR_REQUIRE(d >= 1 && d <= RR_FM64_XT_MAX_DIM, "rr_featmat64_glm_xt: needs 1 <= Xdim <= %d, got %d", RR_FM64_XT_MAX_DIM, d);
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "rr_featmat64_glm_xt: bad dtype");
    RR_REQUIRE(col0 >= 0 && col0 + 2 * (int64_t)n <= fm->F, "rr_featmat64_glm_xt: columns out of range");
    const int dpad = rr_fm64_xt_dpad(d);
    RR_REQUIRE(ldx >= dpad, "rr_featmat64_glm_xt: device X needs ldx >= %d for Xdim = %d", dpad, d);
    RR_REQUIRE(dX != nullptr, "rr_featmat64_glm_xt: null X");
    if (d > 128) return rr_fm64_xt_wide(fm, true, dX, x_dtype, ldx, d, n, col0, dT);
    return glm64_grad_t(fm, dX, x_dtype, ldx, d, dpad, n, col0, dT);
}

int rr_featmat64_glm_edphi(rr_featmat64 *fm, int64_t col0, int64_t ncols, double *E) {
    RR_REQUIRE(fm != nullptr && fm->U != nullptr && fm->have_edphi, "rr_featmat64_glm_edphi: call rr_featmat64_glm_step first");
    RR_REQUIRE(E != nullptr && col0 >= 0 && ncols >= 1 && col0 + ncols <= fm->F, "rr_featmat64_glm_edphi: columns out of range");
    rr_ctx *c = fm->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    RR_CHECK_HIP(hipMemcpy2DAsync(E, (size_t)ncols * 8, fm->U + col0, (size_t)fm->ld * 8, (size_t)ncols * 8, (size_t)fm->rows,
                                  hipMemcpyDeviceToHost, c->stream));
    RR_CHECK_HIP(hipStreamSynchronize(c->stream));
    return RR_OK;
}

// out (rows, S) = P W for a host (F, S) float64 matrix: the latent samples of the prediction calls (glm.py:572-620)
int rr_featmat64_project(rr_featmat64 *fm, const double *W, int S, double *out) {
    RR_REQUIRE(fm != nullptr && W != nullptr && out != nullptr && S >= 1 && S < (1 << 24), "rr_featmat64_project: bad argument");
    RR_FM64_REQUIRE_FILLED(fm, "rr_featmat64_project");
    if (fm->rows == 0) return RR_OK;
    rr_ctx *c = fm->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    const int F = fm->F;
    int rc = glm64_scratch(fm, ((int64_t)S + 127) / 128 * 128, 1);
    if (rc != RR_OK) return rc;
    Glm64Scratch &s = *(Glm64Scratch *)fm->glm;
    const int64_t ldw = s.klp, ld = fm->ld, rp = fm->rows_pad;
    fm->have_rows = false;
    fm->have_edphi = false;
    // W goes up zero padded as the B operand (ld, ldw): rows >= F and columns >= S are zeros
    std::vector<double> w((size_t)ld * ldw, 0.0);
    for (int j = 0; j < F; ++j)
        for (int i = 0; i < S; ++i) w[(size_t)j * ldw + i] = W[(size_t)j * S + i];
    RR_CHECK_HIP(hipStreamSynchronize(c->stream));
    RR_CHECK_HIP(hipMemcpy(s.WSt, w.data(), w.size() * 8, hipMemcpyHostToDevice));
    rc = rr_launch_transpose_f64(c, fm->P, fm->rows, ld, fm->Pt, fm->max_rows, ld, rp);
    if (rc == RR_OK) rc = rr_launch_gemm_tn_f64(c, fm->Pt, fm->max_rows, s.WSt, ldw, s.FS, ldw, ld, rp, ldw, 0, 0);
    if (rc != RR_OK) return rc;
    RR_CHECK_HIP(hipMemcpy2DAsync(out, (size_t)S * 8, s.FS, (size_t)ldw * 8, (size_t)S * 8, (size_t)fm->rows, hipMemcpyDeviceToHost,
                                  c->stream));
    RR_CHECK_HIP(hipStreamSynchronize(c->stream));
    return RR_OK;
}

}  // extern "C"
