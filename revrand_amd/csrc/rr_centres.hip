// Bases defined by a set of centres -- RadialBasis and SigmoidalBasis (basis_functions.py:616-815) -- and PolynomialBasis
// (basis_functions.py:496-576) on the device.  With x_n a row of X, c_j a centre, l the length scale(s):
//   radial:   z = sum_i ((x_ni - c_ji) s_i)^2, s_i = 1 / (2 l_i^2);  Phi = exp(-z)            (:685-686; the reference divides X
//             and C by 2 l^2 BEFORE the squared distance, so the exponent is |x - c|^2 / (4 l^4) -- kept)
//             dPhi_i = Phi ((x_ni - c_ji) / l_i^3)^2                                          (:712-719)
//   sigmoid:  r = sqrt(sum_i ((x_ni - c_ji) / l_i)^2);  Phi = 1 / (1 + exp(-r))               (:784)
//             dPhi_i = -(|x_ni - c_ji| / l_i^2) Phi (1 - Phi)                                 (:809-815)
// An isotropic length scale (n_ls == 1) is used for every dimension of Phi, and its gradient is input dimension 0's term
// only -- the reference's loop runs over the entries of the length-scale vector.
// Distances are always formed from the differences (x - c) s, never from |x|^2 - 2 x.c + |c|^2 (which cancels in f32).
//
// Kernels: features of a row block into a device feature matrix (centre tile in LDS, 16-byte stores); the length-scale
// gradient's contraction sum(E o dPhi_i) against the second pass' / the GLM step's scratch without dPhi, reduced in two
// fixed-order stages (no floating-point atomics); stand-alone transform / grad behind host-buffer entry points; polynomial
// powers into the feature matrix.
#include "rr_internal.h"

namespace {

constexpr int CT = 64;  // centres per tile: 16 lanes x 4 adjacent centres
constexpr int RT = 32;  // rows per sub-tile

struct CentresData {
    int kind = RR_CENTRES_RADIAL;
    int M = 0, Mp = 0;          // centres, row length of the transposed copies (M rounded up to 4)
    float *Ct32 = nullptr;      // (d, Mp): C^T, zero padded -- adjacent lanes read adjacent centres
    double *Ct64 = nullptr;
    // per input dimension, for the length scales in rr_basis::ls_cache (centres_prepare):
    float *scale32 = nullptr;   // s_i: 1 / (2 l_i^2) (radial), 1 / l_i (sigmoid); clamped to a finite float
    double *scale64 = nullptr;
    float *ginv32 = nullptr;    // 1 / l_i^3 (radial), 1 / l_i^2 (sigmoid): the stand-alone grad kernels
    double *ginv64 = nullptr;
};

// What the contraction's sums over (x - c)^2 / |x - c| are multiplied by, 1 / l_i^6 (radial) or 1 / l_i^2 (sigmoid), as a
// kernel argument: made from the length scales the FEATURE MATRIX recorded when the block was put (rr_featmat::centres_puts),
// not from the handle's cache, which the stand-alone transform / grad and puts into other matrices rewrite.
struct GfacArgs {
    double g[128];
};
// (a contraction over more than 128 length scales is one launch per block of 128 of them, each with its own GfacArgs)

template <int KIND, typename T>
__device__ __forceinline__ T centres_phi(T z) {
    if (KIND == RR_CENTRES_RADIAL) return exp(-z);
    return (T)1 / ((T)1 + exp(-sqrt(z)));
}

// ---- features into a feature matrix ------------------------------------------------------------------------------
// A workgroup owns rpb rows x CT columns.  Pa = P + col0 - a with a = col0 & 3, so that column 4 g of a tile is 16-byte
// aligned whatever col0 is: lane group g holds the centres j = tile * CT + 4 g - a + {0..3}, and a group that sticks out of
// [0, M) (the first and last one of the block) stores its valid entries one by one -- neighbouring children's columns and
// the matrix' padding are never touched.  LDS: the centre tile [d][CT], the scales [d], a sub-tile of RT rows [RT][d + 1].
template <typename TX, int KIND>
__global__ void __launch_bounds__(256)
rr_centres_features_kernel(const TX *__restrict__ X, int64_t rows, int64_t ldx, int d, const float *__restrict__ Ct, int Mp, int M,
                           const float *__restrict__ scale, float *__restrict__ Pa, int64_t ldp, int a, int rpb) {
    extern __shared__ __align__(16) float sm[];
    float *cs = sm;
    float *ss = cs + (size_t)d * CT;
    float *xs = ss + ((d + 3) & ~3);
    const int tid = threadIdx.x;
    const int jt0 = (int)blockIdx.y * CT - a;  // centre behind the tile's first column
    for (int e = tid; e < d * CT; e += 256) {
        const int i = e / CT, j = jt0 + (e % CT);
        cs[e] = (j >= 0 && j < M) ? Ct[(size_t)i * Mp + j] : 0.f;
    }
    for (int i = tid; i < d; i += 256) ss[i] = scale[i];
    const int g = tid & 15, rl = tid >> 4;
    const int64_t rb0 = (int64_t)blockIdx.x * rpb;
    const int64_t rb1 = rb0 + rpb < rows ? rb0 + rpb : rows;
    const int xld = d + 1;
    for (int64_t r0 = rb0; r0 < rb1; r0 += RT) {
        __syncthreads();
        for (int e = tid; e < RT * d; e += 256) {
            const int r = e / d, i = e - r * d;
            const int64_t n = r0 + r;
            xs[r * xld + i] = n < rb1 ? (float)X[n * ldx + i] : 0.f;
        }
        __syncthreads();
        float z[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        const float *xa = xs + rl * xld, *xb = xs + (rl + 16) * xld;
        for (int i = 0; i < d; ++i) {
            const float4 c = *reinterpret_cast<const float4 *>(cs + i * CT + 4 * g);
            const float s = ss[i], va = xa[i], vb = xb[i];
            float t;
            t = (va - c.x) * s; z[0][0] = fmaf(t, t, z[0][0]);
            t = (va - c.y) * s; z[0][1] = fmaf(t, t, z[0][1]);
            t = (va - c.z) * s; z[0][2] = fmaf(t, t, z[0][2]);
            t = (va - c.w) * s; z[0][3] = fmaf(t, t, z[0][3]);
            t = (vb - c.x) * s; z[1][0] = fmaf(t, t, z[1][0]);
            t = (vb - c.y) * s; z[1][1] = fmaf(t, t, z[1][1]);
            t = (vb - c.z) * s; z[1][2] = fmaf(t, t, z[1][2]);
            t = (vb - c.w) * s; z[1][3] = fmaf(t, t, z[1][3]);
        }
        const int jb = jt0 + 4 * g;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t n = r0 + rl + 16 * h;
            if (n >= rb1) continue;
            float4 v;
            v.x = centres_phi<KIND, float>(z[h][0]);
            v.y = centres_phi<KIND, float>(z[h][1]);
            v.z = centres_phi<KIND, float>(z[h][2]);
            v.w = centres_phi<KIND, float>(z[h][3]);
            float *dst = Pa + n * ldp + (int64_t)blockIdx.y * CT + 4 * g;
            if (jb >= 0 && jb + 3 < M) {
                RR_DEV_ASSERT(((uintptr_t)dst & 15) == 0);
                *reinterpret_cast<float4 *>(dst) = v;
            } else {
                if (jb >= 0 && jb < M) dst[0] = v.x;
                if (jb + 1 >= 0 && jb + 1 < M) dst[1] = v.y;
                if (jb + 2 >= 0 && jb + 2 < M) dst[2] = v.z;
                if (jb + 3 >= 0 && jb + 3 < M) dst[3] = v.w;
            }
        }
    }
}

// The same for d > 128 (up to RR_CENTRES_MAX_DIM): the dimensions in blocks of DB = 128.  Per sub-tile of RT rows, block after
// block in ascending order, the block's DB rows of the centre tile, its scales and its columns of the RT rows are reloaded into
// the LDS layout above -- [DB][CT], [DB], [RT][DB + 1]: the budget of d = 128, 49.8 KB, three workgroups per compute unit --
// while a lane's eight sums stay in registers.  ONE chain per (row, centre), t = (x - c) s; z = fma(t, t, z) for i = 0 .. d - 1:
// the narrow kernel's sequence, so that no result depends on DB (a column in which x equals c adds exactly 0).  The centre
// block is read again per sub-tile (~64 loads and a barrier against ~3 000 VALU instructions per lane and block; the load phase is
// not overlapped with the arithmetic: 1.18x the narrow kernel's time per term at d = 256, docs/KERNELS.md 3.38).
constexpr int DB = 128;  // dimensions per block

template <typename TX, int KIND>
__global__ void __launch_bounds__(256)
rr_centres_features_wide_kernel(const TX *__restrict__ X, int64_t rows, int64_t ldx, int d, const float *__restrict__ Ct, int Mp, int M,
                                const float *__restrict__ scale, float *__restrict__ Pa, int64_t ldp, int a, int rpb) {
    extern __shared__ __align__(16) float sm[];
    float *cs = sm;                // [DB][CT]
    float *ss = cs + DB * CT;      // [DB]
    float *xs = ss + DB;           // [RT][DB + 1]
    const int tid = threadIdx.x;
    const int jt0 = (int)blockIdx.y * CT - a;  // centre behind the tile's first column
    const int g = tid & 15, rl = tid >> 4;
    const int64_t rb0 = (int64_t)blockIdx.x * rpb;
    const int64_t rb1 = rb0 + rpb < rows ? rb0 + rpb : rows;
    constexpr int xld = DB + 1;
    RR_DEV_ASSERT(d <= ldx);
    for (int64_t r0 = rb0; r0 < rb1; r0 += RT) {
        float z[2][4] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
        for (int i0 = 0; i0 < d; i0 += DB) {
            const int db = d - i0 < DB ? d - i0 : DB;
            RR_DEV_ASSERT(db >= 1 && i0 + db <= d);
            __syncthreads();  // the previous block's (sub-tile's) reads are over
            for (int e = tid; e < db * CT; e += 256) {
                const int i = e / CT, j = jt0 + (e % CT);
                cs[e] = (j >= 0 && j < M) ? Ct[(size_t)(i0 + i) * Mp + j] : 0.f;
            }
            for (int i = tid; i < db; i += 256) ss[i] = scale[i0 + i];
            for (int e = tid; e < RT * db; e += 256) {
                const int r = e / db, i = e - r * db;
                const int64_t n = r0 + r;
                xs[r * xld + i] = n < rb1 ? (float)X[n * ldx + i0 + i] : 0.f;
            }
            __syncthreads();
            const float *xa = xs + rl * xld, *xb = xs + (rl + 16) * xld;
#pragma unroll 4
            for (int i = 0; i < db; ++i) {
                const float4 c = *reinterpret_cast<const float4 *>(cs + i * CT + 4 * g);
                const float s = ss[i], va = xa[i], vb = xb[i];
                float t;
                t = (va - c.x) * s; z[0][0] = fmaf(t, t, z[0][0]);
                t = (va - c.y) * s; z[0][1] = fmaf(t, t, z[0][1]);
                t = (va - c.z) * s; z[0][2] = fmaf(t, t, z[0][2]);
                t = (va - c.w) * s; z[0][3] = fmaf(t, t, z[0][3]);
                t = (vb - c.x) * s; z[1][0] = fmaf(t, t, z[1][0]);
                t = (vb - c.y) * s; z[1][1] = fmaf(t, t, z[1][1]);
                t = (vb - c.z) * s; z[1][2] = fmaf(t, t, z[1][2]);
                t = (vb - c.w) * s; z[1][3] = fmaf(t, t, z[1][3]);
            }
        }
        const int jb = jt0 + 4 * g;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int64_t n = r0 + rl + 16 * h;
            if (n >= rb1) continue;
            float4 v;
            v.x = centres_phi<KIND, float>(z[h][0]);
            v.y = centres_phi<KIND, float>(z[h][1]);
            v.z = centres_phi<KIND, float>(z[h][2]);
            v.w = centres_phi<KIND, float>(z[h][3]);
            float *dst = Pa + n * ldp + (int64_t)blockIdx.y * CT + 4 * g;
            if (jb >= 0 && jb + 3 < M) {
                RR_DEV_ASSERT(((uintptr_t)dst & 15) == 0);
                *reinterpret_cast<float4 *>(dst) = v;
            } else {
                if (jb >= 0 && jb < M) dst[0] = v.x;
                if (jb + 1 >= 0 && jb + 1 < M) dst[1] = v.y;
                if (jb + 2 >= 0 && jb + 2 < M) dst[2] = v.z;
                if (jb + 3 >= 0 && jb + 3 < M) dst[3] = v.w;
            }
        }
    }
}

// ---- the length-scale gradient's contraction ---------------------------------------------------------------------
// g_i = sum_{n,j} E_nj dPhi_i[n,j] for the nd = n_ls entries of the length-scale vector (isotropic: input dimension 0
// only), with E = err m^T - U (SLM, slm.py:193-195) or E = U = EdPhi (GLM, glm.py:274-275).  The factor common to every
// dimension is formed once per entry, w = E Phi (radial) or w = -E Phi (1 - Phi) (sigmoid), and kept in LDS; what is
// left per dimension is sum w (x_i - c_i)^2 (radial) or sum w |x_i - c_i| (sigmoid), times gfac_i at the very end.
// Thread (i, slice): dimension i = tid % DP (DP = nd rounded up to a power of two), and every (256 / DP)-th of the
// RT x 16 (row, four centres) units of a sub-tile.  Four products are summed in f32, everything beyond that in float64:
// per thread across the block's rows, across the slices in slice order, and the block's nd sums go to
// partial[block][i] -- the second stage (rr_det_reduce) adds the blocks in index order.  No atomics anywhere.
template <typename TX, int KIND, bool SLM>
__global__ void __launch_bounds__(256)
rr_centres_contract_kernel(const TX *__restrict__ X, int64_t rows, int64_t ldx, int nd, int DP, const float *__restrict__ Ct, int Mp,
                           int M, const float *__restrict__ P, const float *__restrict__ U, int64_t ldp,
                           const float *__restrict__ err, const float *__restrict__ mvec, const GfacArgs gfac, int rpb,
                           double *__restrict__ partial) {
    extern __shared__ __align__(16) float sm[];
    float4 *cs4 = reinterpret_cast<float4 *>(sm);  // [16][DP]: centres 4 q4 .. 4 q4 + 3 of dimension i
    float4 *ws4 = cs4 + 16 * DP;                   // [RT][16]
    float *xs = reinterpret_cast<float *>(ws4 + RT * 16);  // [RT][DP + 1]
    __shared__ double red[256];
    const int tid = threadIdx.x;
    const int i = tid & (DP - 1), slice = tid / DP, nsl = 256 / DP;
    const int j0 = (int)blockIdx.y * CT;
    for (int e = tid; e < 16 * DP; e += 256) {
        const int q4 = e / DP, ii = e - q4 * DP;
        float c[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int j = j0 + 4 * q4 + q;
            c[q] = (ii < nd && j < M) ? Ct[(size_t)ii * Mp + j] : 0.f;
        }
        cs4[e] = make_float4(c[0], c[1], c[2], c[3]);
    }
    const int64_t rb0 = (int64_t)blockIdx.x * rpb;
    const int64_t rb1 = rb0 + rpb < rows ? rb0 + rpb : rows;
    const int xld = DP + 1;
    double acc = 0.0;
    for (int64_t r0 = rb0; r0 < rb1; r0 += RT) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RT * CT / 256; ++k) {
            const int e = tid + 256 * k, r = e >> 6, j = j0 + (e & 63);
            const int64_t n = r0 + r;
            float w = 0.f;
            if (n < rb1 && j < M) {
                RR_DEV_ASSERT(j < ldp);
                const float phi = P[n * ldp + j], u = U[n * ldp + j];
                const float E = SLM ? fmaf(err[n], mvec[j], -u) : u;
                w = KIND == RR_CENTRES_RADIAL ? E * phi : -E * phi * (1.f - phi);
            }
            reinterpret_cast<float *>(ws4)[e] = w;
        }
        for (int e = tid; e < RT * DP; e += 256) {
            const int r = e / DP, ii = e - r * DP;
            const int64_t n = r0 + r;
            xs[r * xld + ii] = (n < rb1 && ii < nd) ? (float)X[n * ldx + ii] : 0.f;
        }
        __syncthreads();
        for (int u = slice; u < RT * 16; u += nsl) {
            const float4 w = ws4[u], c = cs4[(u & 15) * DP + i];
            const float x = xs[(u >> 4) * xld + i];
            float s;
            if (KIND == RR_CENTRES_RADIAL) {
                const float t0 = x - c.x, t1 = x - c.y, t2 = x - c.z, t3 = x - c.w;
                s = fmaf(w.x * t0, t0, fmaf(w.y * t1, t1, fmaf(w.z * t2, t2, w.w * t3 * t3)));
            } else {
                s = fmaf(w.x, fabsf(x - c.x), fmaf(w.y, fabsf(x - c.y), fmaf(w.z, fabsf(x - c.z), w.w * fabsf(x - c.w))));
            }
            acc += (double)s;
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (tid < nd) {
        double s = 0.0;
        for (int sl = 0; sl < nsl; ++sl) s += red[sl * DP + tid];
        partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nd + tid] = s * gfac.g[tid];
    }
}

// ---- stand-alone transform / grad (device chunk buffers of the host entry points) --------------------------------
// One thread per (row, centre), centres adjacent across lanes (C^T is read coalesced, x broadcast); arithmetic in T,
// results stored as float64.  These calls are bound by the copy of their (N, M[, d]) float64 result to the host.
template <typename TX, typename T, int KIND>
__global__ void __launch_bounds__(256)
rr_centres_transform_kernel(const TX *__restrict__ X, int64_t m, int64_t ldx, int d, const T *__restrict__ Ct, int Mp, int M,
                            const T *__restrict__ scale, double *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * M) return;
    const int64_t n = idx / M;
    const int j = (int)(idx - n * M);
    T z = 0;
    for (int i = 0; i < d; ++i) {
        const T t = ((T)X[n * ldx + i] - Ct[(size_t)i * Mp + j]) * scale[i];
        z += t * t;
    }
    out[idx] = (double)centres_phi<KIND, T>(z);
}

// n_ls == 1: out (m, M), dimension 0's term; else out (m, M, d) -- the reference's np.dstack layout, written directly
template <typename TX, typename T, int KIND>
__global__ void __launch_bounds__(256)
rr_centres_grad_kernel(const TX *__restrict__ X, int64_t m, int64_t ldx, int d, int n_ls, const T *__restrict__ Ct, int Mp, int M,
                       const T *__restrict__ scale, const T *__restrict__ ginv, double *__restrict__ out) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= m * M) return;
    const int64_t n = idx / M;
    const int j = (int)(idx - n * M);
    T z = 0;
    for (int i = 0; i < d; ++i) {
        const T t = ((T)X[n * ldx + i] - Ct[(size_t)i * Mp + j]) * scale[i];
        z += t * t;
    }
    const T phi = centres_phi<KIND, T>(z);
    const T common = KIND == RR_CENTRES_RADIAL ? phi : -phi * ((T)1 - phi);
    double *o = out + idx * n_ls;
    for (int i = 0; i < n_ls; ++i) {
        const T t = ((T)X[n * ldx + i] - Ct[(size_t)i * Mp + j]) * ginv[i];
        o[i] = (double)(common * (KIND == RR_CENTRES_RADIAL ? t * t : fabs(t)));
    }
}

// ---- PolynomialBasis.transform (basis_functions.py:549-567) into a feature matrix ---------------------------------
// [1] (bias), then for input dimension i the powers x_i^1 .. x_i^order at columns bias + i order + p - 1: one thread per
// (row, dimension), powers by repeated multiplication
template <typename TX>
__global__ void __launch_bounds__(256)
rr_poly_features_kernel(const TX *__restrict__ X, int64_t N, int64_t ldx, int d, int order, int bias, float *__restrict__ P,
                        int64_t ldp) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= N * d) return;
    const int64_t r = t / d;
    const int i = (int)(t - r * d);
    RR_DEV_ASSERT(bias + (int64_t)d * order <= ldp && d <= ldx);
    float *row = P + r * ldp;
    if (bias && i == 0) row[0] = 1.f;
    const float x = (float)X[r * ldx + i];
    float p = 1.f;
    for (int k = 0; k < order; ++k) {
        p *= x;
        row[bias + i * order + k] = p;
    }
}

// ---- the same three kernels in FLOAT64, for the float64 feature matrix (rr_featmat64, rr_elbo.hip) --------------------------
// Every product and sum is float64, from Ct64 and the UNCLAMPED scale64 of centres_prepare (as the stand-alone float64
// transform).  The centre tile is HALF the f32 kernels': CT64 = 32 centres = 16 lanes x 2 adjacent centres, so that a lane's
// store is still 16 bytes (two doubles) and the d = 128 workgroup stays under 64 KiB of LDS (three per compute unit, as in
// f32) instead of the 98 KB -- one workgroup per compute unit -- the f32 tile would take in doubles.
constexpr int CT64 = 32;  // centres per tile: 16 lanes x 2 adjacent centres
constexpr int RT64 = 16;  // rows per sub-tile: one row per thread

// A workgroup owns rpb rows x CT64 columns.  Pa = P + col0 - a with a = col0 & 1, so that column 2 g of a tile is 16-byte
// aligned whatever col0 is: lane group g holds the centres j = tile * CT64 + 2 g - a + {0, 1}; a pair that sticks out of
// [0, M) stores its valid entry alone.  cmax = the columns of a row from Pa on (the matrix' ld - (col0 - a)).
// LDS (doubles): the centre tile [d][CT64], the scales [d rounded up to 2], a sub-tile of RT64 rows [RT64][d + 1].
template <typename TX, int KIND>
__global__ void __launch_bounds__(256)
rr_centres_features64_kernel(const TX *__restrict__ X, int64_t rows, int64_t ldx, int d, const double *__restrict__ Ct, int Mp, int M,
                             const double *__restrict__ scale, double *__restrict__ Pa, int64_t ldp, int a, int rpb, int64_t cmax) {
    extern __shared__ __align__(16) double smd[];
    double *cs = smd;
    double *ss = cs + (size_t)d * CT64;
    double *xs = ss + ((d + 1) & ~1);
    const int tid = threadIdx.x;
    const int jt0 = (int)blockIdx.y * CT64 - a;  // centre behind the tile's first column
    for (int e = tid; e < d * CT64; e += 256) {
        const int i = e / CT64, j = jt0 + (e % CT64);
        cs[e] = (j >= 0 && j < M) ? Ct[(size_t)i * Mp + j] : 0.0;
    }
    for (int i = tid; i < d; i += 256) ss[i] = scale[i];
    const int g = tid & 15, rl = tid >> 4;
    const int64_t rb0 = (int64_t)blockIdx.x * rpb;
    const int64_t rb1 = rb0 + rpb < rows ? rb0 + rpb : rows;
    const int xld = d + 1;
    for (int64_t r0 = rb0; r0 < rb1; r0 += RT64) {
        __syncthreads();
        for (int e = tid; e < RT64 * d; e += 256) {
            const int r = e / d, i = e - r * d;
            const int64_t n = r0 + r;
            RR_DEV_ASSERT(d <= ldx);
            xs[r * xld + i] = n < rb1 ? (double)X[n * ldx + i] : 0.0;
        }
        __syncthreads();
        double z0 = 0.0, z1 = 0.0;
        const double *xa = xs + rl * xld;
        for (int i = 0; i < d; ++i) {
            const double2 c = *reinterpret_cast<const double2 *>(cs + i * CT64 + 2 * g);
            const double s = ss[i], v = xa[i];
            double t;
            t = (v - c.x) * s; z0 = fma(t, t, z0);
            t = (v - c.y) * s; z1 = fma(t, t, z1);
        }
        const int64_t n = r0 + rl;
        if (n >= rb1) continue;
        const int jb = jt0 + 2 * g;
        const int64_t col = (int64_t)blockIdx.y * CT64 + 2 * g;
        double2 v;
        v.x = centres_phi<KIND, double>(z0);
        v.y = centres_phi<KIND, double>(z1);
        double *dst = Pa + n * ldp + col;
        if (jb >= 0 && jb + 1 < M) {
            RR_DEV_ASSERT(((uintptr_t)dst & 15) == 0 && col + 2 <= cmax);
            *reinterpret_cast<double2 *>(dst) = v;
        } else {
            if (jb >= 0 && jb < M) {
                RR_DEV_ASSERT(col < cmax);
                dst[0] = v.x;
            }
            if (jb + 1 >= 0 && jb + 1 < M) {
                RR_DEV_ASSERT(col + 1 < cmax);
                dst[1] = v.y;
            }
        }
    }
}

// rr_centres_features64_kernel for d > 128: the dimensions in blocks of DB, as rr_centres_features_wide_kernel -- the block's
// centre rows [DB][CT64], scales [DB] and row sub-tile [RT64][DB + 1] in the LDS budget of d = 128 (50.3 KB), a lane's two
// sums in registers across the blocks, one ascending fma chain per (row, centre).
template <typename TX, int KIND>
__global__ void __launch_bounds__(256)
rr_centres_features64_wide_kernel(const TX *__restrict__ X, int64_t rows, int64_t ldx, int d, const double *__restrict__ Ct, int Mp, int M,
                                  const double *__restrict__ scale, double *__restrict__ Pa, int64_t ldp, int a, int rpb, int64_t cmax) {
    extern __shared__ __align__(16) double smd[];
    double *cs = smd;               // [DB][CT64]
    double *ss = cs + DB * CT64;    // [DB]
    double *xs = ss + DB;           // [RT64][DB + 1]
    const int tid = threadIdx.x;
    const int jt0 = (int)blockIdx.y * CT64 - a;  // centre behind the tile's first column
    const int g = tid & 15, rl = tid >> 4;
    const int64_t rb0 = (int64_t)blockIdx.x * rpb;
    const int64_t rb1 = rb0 + rpb < rows ? rb0 + rpb : rows;
    constexpr int xld = DB + 1;
    RR_DEV_ASSERT(d <= ldx);
    for (int64_t r0 = rb0; r0 < rb1; r0 += RT64) {
        double z0 = 0.0, z1 = 0.0;
        for (int i0 = 0; i0 < d; i0 += DB) {
            const int db = d - i0 < DB ? d - i0 : DB;
            RR_DEV_ASSERT(db >= 1 && i0 + db <= d);
            __syncthreads();  // the previous block's (sub-tile's) reads are over
            for (int e = tid; e < db * CT64; e += 256) {
                const int i = e / CT64, j = jt0 + (e % CT64);
                cs[e] = (j >= 0 && j < M) ? Ct[(size_t)(i0 + i) * Mp + j] : 0.0;
            }
            for (int i = tid; i < db; i += 256) ss[i] = scale[i0 + i];
            for (int e = tid; e < RT64 * db; e += 256) {
                const int r = e / db, i = e - r * db;
                const int64_t n = r0 + r;
                xs[r * xld + i] = n < rb1 ? (double)X[n * ldx + i0 + i] : 0.0;
            }
            __syncthreads();
            const double *xa = xs + rl * xld;
#pragma unroll 4
            for (int i = 0; i < db; ++i) {
                const double2 c = *reinterpret_cast<const double2 *>(cs + i * CT64 + 2 * g);
                const double s = ss[i], v = xa[i];
                double t;
                t = (v - c.x) * s; z0 = fma(t, t, z0);
                t = (v - c.y) * s; z1 = fma(t, t, z1);
            }
        }
        const int64_t n = r0 + rl;
        if (n >= rb1) continue;
        const int jb = jt0 + 2 * g;
        const int64_t col = (int64_t)blockIdx.y * CT64 + 2 * g;
        double2 v;
        v.x = centres_phi<KIND, double>(z0);
        v.y = centres_phi<KIND, double>(z1);
        double *dst = Pa + n * ldp + col;
        if (jb >= 0 && jb + 1 < M) {
            RR_DEV_ASSERT(((uintptr_t)dst & 15) == 0 && col + 2 <= cmax);
            *reinterpret_cast<double2 *>(dst) = v;
        } else {
            if (jb >= 0 && jb < M) {
                RR_DEV_ASSERT(col < cmax);
                dst[0] = v.x;
            }
            if (jb + 1 >= 0 && jb + 1 < M) {
                RR_DEV_ASSERT(col + 1 < cmax);
                dst[1] = v.y;
            }
        }
    }
}

// rr_centres_contract_kernel<..., SLM = true> in float64: E = err m^T - U against the float64 matrix' P, U, err and m.  The same
// decomposition -- w = E Phi (radial) or -E Phi (1 - Phi) (sigmoid) per entry in LDS, then per dimension sum w (x_i - c_i)^2 or
// sum w |x_i - c_i|, times gfac_i at the end -- on tiles of RT64 rows x CT64 centres in units of (row, two centres).  Thread
// (i, slice) as there; every product and sum is float64, added in a fixed order: per thread over its units and the block's
// rows, across the slices in slice order, the block's nd sums to partial[block][i] (then rr_det_reduce).  No atomics.
// LDS (all dynamic): centres [16][DP] double2, w [RT64][CT64], rows [RT64][DP + 1], the slices' sums [256].
// SLM = false (the float64 GLM step, rr_featmat64_glm_centres): E = U, the step's EdPhi; err and mvec are not read.
template <typename TX, int KIND, bool SLM = true>
__global__ void __launch_bounds__(256)
rr_centres_contract64_kernel(const TX *__restrict__ X, int64_t rows, int64_t ldx, int nd, int DP, const double *__restrict__ Ct, int Mp,
                             int M, const double *__restrict__ P, const double *__restrict__ U, int64_t ldp,
                             const double *__restrict__ err, const double *__restrict__ mvec, const GfacArgs gfac, int rpb,
                             double *__restrict__ partial) {
    extern __shared__ __align__(16) double smd[];
    double2 *cs2 = reinterpret_cast<double2 *>(smd);  // [16][DP]: centres 2 q2, 2 q2 + 1 of dimension i
    double *ws = smd + 2 * 16 * DP;                  // [RT64][CT64]
    double *xs = ws + RT64 * CT64;                   // [RT64][DP + 1]
    double *red = xs + RT64 * (DP + 1);              // [256]
    const int tid = threadIdx.x;
    const int i = tid & (DP - 1), slice = tid / DP, nsl = 256 / DP;
    const int j0 = (int)blockIdx.y * CT64;
    for (int e = tid; e < 16 * DP; e += 256) {
        const int q2 = e / DP, ii = e - q2 * DP;
        const int j = j0 + 2 * q2;
        double2 c;
        c.x = (ii < nd && j < M) ? Ct[(size_t)ii * Mp + j] : 0.0;
        c.y = (ii < nd && j + 1 < M) ? Ct[(size_t)ii * Mp + j + 1] : 0.0;
        cs2[e] = c;
    }
    const int64_t rb0 = (int64_t)blockIdx.x * rpb;
    const int64_t rb1 = rb0 + rpb < rows ? rb0 + rpb : rows;
    const int xld = DP + 1;
    double acc = 0.0;
    for (int64_t r0 = rb0; r0 < rb1; r0 += RT64) {
        __syncthreads();
#pragma unroll
        for (int k = 0; k < RT64 * CT64 / 256; ++k) {
            const int e = tid + 256 * k, r = e >> 5, j = j0 + (e & 31);
            const int64_t n = r0 + r;
            double w = 0.0;
            if (n < rb1 && j < M) {
                RR_DEV_ASSERT(j < ldp);
                const double phi = P[n * ldp + j], u = U[n * ldp + j];
                const double E = SLM ? fma(err[n], mvec[j], -u) : u;
                w = KIND == RR_CENTRES_RADIAL ? E * phi : -E * phi * (1.0 - phi);
            }
            ws[e] = w;
        }
        for (int e = tid; e < RT64 * DP; e += 256) {
            const int r = e / DP, ii = e - r * DP;
            const int64_t n = r0 + r;
            RR_DEV_ASSERT(nd <= ldx);
            xs[r * xld + ii] = (n < rb1 && ii < nd) ? (double)X[n * ldx + ii] : 0.0;
        }
        __syncthreads();
        for (int u = slice; u < RT64 * 16; u += nsl) {
            const double2 w = *reinterpret_cast<const double2 *>(ws + 2 * u), c = cs2[(u & 15) * DP + i];
            const double x = xs[(u >> 4) * xld + i];
            double s;
            if (KIND == RR_CENTRES_RADIAL) {
                const double t0 = x - c.x, t1 = x - c.y;
                s = fma(w.x * t0, t0, w.y * t1 * t1);
            } else {
                s = fma(w.x, fabs(x - c.x), w.y * fabs(x - c.y));
            }
            acc += s;
        }
    }
    red[tid] = acc;
    __syncthreads();
    if (tid < nd) {
        double s = 0.0;
        for (int sl = 0; sl < nsl; ++sl) s += red[sl * DP + tid];
        partial[((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * nd + tid] = s * gfac.g[tid];
    }
}

// rr_poly_features_kernel into the float64 matrix: the powers by repeated multiplication in float64
template <typename TX>
__global__ void __launch_bounds__(256)
rr_poly_features64_kernel(const TX *__restrict__ X, int64_t N, int64_t ldx, int d, int order, int bias, double *__restrict__ P,
                          int64_t ldp) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= N * d) return;
    const int64_t r = t / d;
    const int i = (int)(t - r * d);
    RR_DEV_ASSERT(bias + (int64_t)d * order <= ldp && d <= ldx);
    double *row = P + r * ldp;
    if (bias && i == 0) row[0] = 1.0;
    const double x = (double)X[r * ldx + i];
    double p = 1.0;
    for (int k = 0; k < order; ++k) {
        p *= x;
        row[bias + i * order + k] = p;
    }
}

// ---- the resident SVI loop's side (rr_glm_sgd, rr_elbo.hip) --------------------------------------------------------
// The d float32 feature scales of centres_prepare from the child's float64 length scales in HBM (the loop's x, after
// rr_glm_sgd_from_log_kernel): the same clamp and isotropic broadcast, into a buffer the LOOP owns.  A zero length scale gives
// the clamped +-1e18, a NaN stays a NaN: nothing can be refused from inside a queued step.
__global__ void __launch_bounds__(128)
rr_centres_scale_dev_kernel(const double *__restrict__ ls, int n_ls, int d, int radial, float *__restrict__ scale) {
#pragma clang fp contract(off)
    const int i = (int)blockIdx.x * 128 + (int)threadIdx.x;
    if (i >= d) return;
    const double l = ls[n_ls == 1 ? 0 : i];
    const double s = radial ? 1.0 / (2.0 * l * l) : 1.0 / l;
    const double lim = 1e18;
    scale[i] = (float)(s > lim ? lim : (s < -lim ? -lim : s));
}

CentresData *centres_of(rr_basis *b) { return b != nullptr && b->kind == RR_KIND_CENTRES ? (CentresData *)b->centres : nullptr; }

// The per-dimension factors for these length scales, cached like rr_basis_prepare caches the scaled W
int centres_prepare(rr_basis *b, const double *lenscale, int n_ls, const char *who) {
    CentresData *cd = centres_of(b);
    RR_REQUIRE(cd != nullptr, "%s: not a centres basis", who);
    RR_REQUIRE(lenscale != nullptr && (n_ls == 1 || n_ls == b->d), "%s: need 1 or d=%d length scales, got %d", who, b->d, n_ls);
    if ((int)b->ls_cache.size() == n_ls && memcmp(b->ls_cache.data(), lenscale, (size_t)n_ls * 8) == 0) return RR_OK;
    const int d = b->d;
    std::vector<float> s32((size_t)d), g32((size_t)d);
    std::vector<double> s64((size_t)d), g64((size_t)d);
    // The optimiser's log-space bounds let a length scale reach 1e-100: the float32 factors are clamped to a finite range
    // (like the random Fourier kernels' scaled W), so that (x - c) s is never 0 * inf; z then overflows to inf and Phi
    // is exp(-inf) = 0 or 1 as in the reference's float64.
    const double lim = 1e18;
    for (int i = 0; i < d; ++i) {
        const double l = lenscale[n_ls == 1 ? 0 : i];
        RR_REQUIRE(l != 0.0 && l == l, "%s: lenscale[%d] is %g", who, i, l);
        const bool radial = cd->kind == RR_CENTRES_RADIAL;
        s64[i] = radial ? 1.0 / (2.0 * l * l) : 1.0 / l;
        g64[i] = radial ? 1.0 / (l * l * l) : 1.0 / (l * l);
        s32[i] = (float)(s64[i] > lim ? lim : (s64[i] < -lim ? -lim : s64[i]));
        g32[i] = (float)(g64[i] > lim ? lim : (g64[i] < -lim ? -lim : g64[i]));
    }
    RR_CHECK_HIP(hipSetDevice(b->ctx->device));
    RR_CHECK_HIP(hipStreamSynchronize(b->ctx->stream));  // kernels in flight read the old factors
    b->ls_cache.clear();
    RR_CHECK_HIP(hipMemcpy(cd->scale32, s32.data(), (size_t)d * 4, hipMemcpyHostToDevice));
    RR_CHECK_HIP(hipMemcpy(cd->ginv32, g32.data(), (size_t)d * 4, hipMemcpyHostToDevice));
    RR_CHECK_HIP(hipMemcpy(cd->scale64, s64.data(), (size_t)d * 8, hipMemcpyHostToDevice));
    RR_CHECK_HIP(hipMemcpy(cd->ginv64, g64.data(), (size_t)d * 8, hipMemcpyHostToDevice));
    b->ls_cache.assign(lenscale, lenscale + n_ls);
    return RR_OK;
}

template <typename TX, typename T, int KIND, bool GRAD>
void centres_launch_host_kernel(rr_basis *b, CentresData *cd, const void *dX, int64_t m, int n_ls, double *dO) {
    const T *Ct = sizeof(T) == 4 ? (const T *)cd->Ct32 : (const T *)cd->Ct64;
    const T *sc = sizeof(T) == 4 ? (const T *)cd->scale32 : (const T *)cd->scale64;
    const T *gi = sizeof(T) == 4 ? (const T *)cd->ginv32 : (const T *)cd->ginv64;
    const dim3 grid((unsigned)((m * cd->M + 255) / 256));
    if (GRAD)
        hipLaunchKernelGGL((rr_centres_grad_kernel<TX, T, KIND>), grid, dim3(256), 0, b->ctx->stream, (const TX *)dX, m,
                           (int64_t)b->d, b->d, n_ls, Ct, cd->Mp, cd->M, sc, gi, dO);
    else
        hipLaunchKernelGGL((rr_centres_transform_kernel<TX, T, KIND>), grid, dim3(256), 0, b->ctx->stream, (const TX *)dX, m,
                           (int64_t)b->d, b->d, Ct, cd->Mp, cd->M, sc, dO);
}

template <bool GRAD>
void centres_dispatch_host_kernel(rr_basis *b, CentresData *cd, const void *dX, int x_dtype, int64_t m, int n_ls, double *dO) {
#define RR_CK(TX, T)                                                                                           \
    if (cd->kind == RR_CENTRES_RADIAL) centres_launch_host_kernel<TX, T, RR_CENTRES_RADIAL, GRAD>(b, cd, dX, m, n_ls, dO); \
    else centres_launch_host_kernel<TX, T, RR_CENTRES_SIGMOID, GRAD>(b, cd, dX, m, n_ls, dO)
    if (b->compute == RR_F32) {
        if (x_dtype == RR_F32) { RR_CK(float, float); } else { RR_CK(double, float); }
    } else {
        if (x_dtype == RR_F32) { RR_CK(float, double); } else { RR_CK(double, double); }
    }
#undef RR_CK
}

// common host-buffer driver: stream row chunks up, run the kernel, stream the float64 result down (rr_host_sink)
template <bool GRAD>
int centres_host_call(rr_basis *b, const void *X, int x_dtype, int64_t N, int64_t ldx, const double *lenscale, int n_ls,
                      double *out, const char *who) {
    CentresData *cd = centres_of(b);
    RR_REQUIRE(cd != nullptr, "%s: not a centres basis", who);
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "%s: bad dtype", who);
    RR_REQUIRE(N >= 0 && ldx >= b->d, "%s: bad shape", who);
    rr_ctx *c = b->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    int rc = centres_prepare(b, lenscale, n_ls, who);
    if (rc != RR_OK || N == 0) return rc;
    RR_REQUIRE(X != nullptr && out != nullptr, "%s: null buffer", who);
    const size_t xs = x_dtype == RR_F32 ? 4 : 8;
    const size_t width = (size_t)cd->M * (GRAD ? (size_t)n_ls : 1);
    int64_t chunk = (int64_t)(((size_t)256 << 20) / ((size_t)b->d * xs + width * 8));  // pipelined chunks
    if (chunk < 1) chunk = 1;
    if (chunk > N) chunk = N;
    void *dX = nullptr, *dO = nullptr;
    if (hipMalloc(&dX, (size_t)chunk * b->d * xs) != hipSuccess || hipMalloc(&dO, (size_t)chunk * width * 8) != hipSuccess) {
        (void)hipGetLastError();
        if (dX) (void)hipFree(dX);
        rr_set_error("%s: device allocation failed", who);
        return RR_ERR_OOM;
    }
    rr_host_sink sink;
    rc = rr_sink_open(c, (size_t)chunk * width * 8, &sink);
    for (int64_t r0 = 0; r0 < N && rc == RR_OK; r0 += chunk) {
        const int64_t m = (N - r0 < chunk) ? N - r0 : chunk;
        hipError_t e = hipMemcpy2DAsync(dX, (size_t)b->d * xs, (const char *)X + (size_t)r0 * ldx * xs, (size_t)ldx * xs,
                                        (size_t)b->d * xs, (size_t)m, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) {
            centres_dispatch_host_kernel<GRAD>(b, cd, dX, x_dtype, m, n_ls, (double *)dO);
            e = hipGetLastError();
        }
        if (e != hipSuccess) {
            rr_set_error("%s: chunk at row %lld failed: %s", who, (long long)r0, hipGetErrorString(e));
            rc = RR_ERR_HIP;
            break;
        }
        rc = rr_sink_push(&sink, dO, (char *)out + (size_t)r0 * width * 8, (size_t)m, width * 8, width * 8);
    }
    if (rc == RR_OK) rc = rr_sink_close(&sink);
    (void)hipStreamSynchronize(c->stream);
    (void)hipFree(dX);
    (void)hipFree(dO);
    return rc;
}

// the contraction's launch and its second stage for the nd <= 128 length scales i0 .. i0 + nd - 1:
// dg[i0 + i] += gfac.g[i] * (the block sums in index order), i < nd.  The per-dimension sums are independent of each other, so
// the kernel sees columns i0 .. of X and rows i0 .. of C^T as its dimensions 0 .. nd - 1 (rr_grad_t_kernel's pattern for
// Xdim > 128); w = E o Phi is formed again per launch.
template <bool SLM>
int centres_contract_launch(rr_featmat *fm, CentresData *cd, const void *dX, int x_dtype, int64_t ldx, int64_t col0, int i0, int nd,
                            const GfacArgs &gfac, double *dg) {
    float *U = nullptr, *err = nullptr, *m32 = nullptr;
    bool have_rows = false, have_edphi = false;
    rr_fm_pass2_views(fm->pass2, &U, &err, &m32, &have_rows, &have_edphi);
    rr_ctx *c = fm->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    int DP = 1;
    while (DP < nd) DP *= 2;
    const int ctiles = (cd->M + CT - 1) / CT;
    // about 8 workgroups per compute unit, whole sub-tiles of rows each: few enough partial sums for the second stage
    int64_t rpb = (fm->rows * ctiles + (int64_t)c->num_cu * 8 - 1) / ((int64_t)c->num_cu * 8);
    rpb = (rpb + RT - 1) / RT * RT;
    const dim3 grid((unsigned)((fm->rows + rpb - 1) / rpb), (unsigned)ctiles);
    const int64_t nblocks = (int64_t)grid.x * grid.y;
    void *part = nullptr;
    int rc = rr_det_scratch(c, (size_t)nblocks * nd * 8, &part);
    if (rc != RR_OK) return rc;
    const size_t lds = (size_t)16 * DP * 16 + (size_t)RT * 16 * 16 + (size_t)RT * (DP + 1) * 4;
    const float *P = fm->P + col0, *Uc = U + col0, *mv = m32 + col0;
    const float *Ct = cd->Ct32 + (size_t)i0 * cd->Mp;
#define RR_CC(TX, KIND)                                                                                                    \
    hipLaunchKernelGGL((rr_centres_contract_kernel<TX, KIND, SLM>), grid, dim3(256), lds, c->stream, (const TX *)dX + i0, fm->rows, ldx, \
                       nd, DP, Ct, cd->Mp, cd->M, P, Uc, fm->ld, err, mv, gfac, (int)rpb, (double *)part)
    if (cd->kind == RR_CENTRES_RADIAL) {
        if (x_dtype == RR_F32) RR_CC(float, RR_CENTRES_RADIAL);
        else RR_CC(double, RR_CENTRES_RADIAL);
    } else {
        if (x_dtype == RR_F32) RR_CC(float, RR_CENTRES_SIGMOID);
        else RR_CC(double, RR_CENTRES_SIGMOID);
    }
#undef RR_CC
    RR_CHECK_HIP(hipGetLastError());
    return rr_det_reduce(c, (const double *)part, nblocks, nd, nd, dg + i0);
}

// gfac of the length scales ls[i0 .. i0 + 127] (n of them in all): 1 / l^6 (radial), 1 / l^2 (sigmoid); 1 behind the last
void centres_gfac(const CentresData *cd, const std::vector<double> &ls, int i0, GfacArgs *gfac) {
    const int n = (int)ls.size();
    for (int i = 0; i < 128; ++i) {
        const double l = i0 + i < n ? ls[(size_t)(i0 + i)] : 1.0;
        const double g = cd->kind == RR_CENTRES_RADIAL ? 1.0 / (l * l * l) : 1.0 / (l * l);
        gfac->g[i] = cd->kind == RR_CENTRES_RADIAL ? g * g : g;
    }
}

template <bool SLM>
int centres_contract(rr_featmat *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, int64_t col0, double *dg,
                     const char *who) {
    CentresData *cd = centres_of(b);
    RR_REQUIRE(fm != nullptr && cd != nullptr && dg != nullptr, "%s: bad argument", who);
    float *U = nullptr, *err = nullptr, *m32 = nullptr;
    bool have_rows = false, have_edphi = false;
    rr_fm_pass2_views(fm->pass2, &U, &err, &m32, &have_rows, &have_edphi);
    RR_REQUIRE(SLM ? have_rows : have_edphi, "%s: call %s first", who, SLM ? "rr_featmat_pass2_rows" : "rr_featmat_glm_step");
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "%s: bad dtype", who);
    RR_REQUIRE(b->d <= RR_CENTRES_MAX_DIM, "%s: needs d <= %d, got %d", who, RR_CENTRES_MAX_DIM, b->d);
    RR_REQUIRE(col0 >= 0 && col0 + (int64_t)cd->M <= fm->F, "%s: columns out of range", who);
    RR_REQUIRE(ldx >= b->d, "%s: device X needs ldx >= d = %d", who, b->d);
    const std::vector<double> *put_ls = nullptr;
    for (const auto &pc : fm->centres_puts)
        if (pc.basis == b && pc.col0 == col0) put_ls = &pc.ls;
    RR_REQUIRE(put_ls != nullptr, "%s: this basis was not put at column %lld since rr_featmat_begin (rr_featmat_put_centres)", who,
               (long long)col0);
    if (fm->rows == 0) return RR_OK;
    RR_REQUIRE(dX != nullptr, "%s: null X", who);
    const int nd = (int)put_ls->size();
    RR_REQUIRE(nd == 1 || nd == b->d, "%s: the block was put with %d length scales, d = %d", who, nd, b->d);
    for (int i0 = 0; i0 < nd; i0 += 128) {  // (isotropic: dimension 0 alone, one launch)
        GfacArgs gfac;
        centres_gfac(cd, *put_ls, i0, &gfac);
        const int rc = centres_contract_launch<SLM>(fm, cd, dX, x_dtype, ldx, col0, i0, nd - i0 < 128 ? nd - i0 : 128, gfac, dg);
        if (rc != RR_OK) return rc;
    }
    return RR_OK;
}

// features of fm's rows at col0 with the d float32 scales at `scale` (device), on the context's stream
void centres_launch_features(rr_featmat *fm, const CentresData *cd, int d, const void *dX, int x_dtype, int64_t ldx,
                             const float *scale, int64_t col0) {
    const int a = (int)(col0 & 3);
    const int rpb = 256;
    const dim3 grid((unsigned)((fm->rows + rpb - 1) / rpb), (unsigned)((a + cd->M + CT - 1) / CT));
    const bool wide = d > DB;  // dimension blocks; the LDS of d = DB
    const int dl = wide ? DB : d;
    const size_t lds = ((size_t)dl * CT + (size_t)((dl + 3) & ~3) + (size_t)RT * (dl + 1)) * 4;
    float *Pa = fm->P + (col0 - a);
#define RR_CF(TX, KIND)                                                                                                        \
    if (wide)                                                                                                                  \
        hipLaunchKernelGGL((rr_centres_features_wide_kernel<TX, KIND>), grid, dim3(256), lds, fm->ctx->stream, (const TX *)dX, fm->rows, \
                           ldx, d, cd->Ct32, cd->Mp, cd->M, scale, Pa, fm->ld, a, rpb);                                        \
    else                                                                                                                       \
        hipLaunchKernelGGL((rr_centres_features_kernel<TX, KIND>), grid, dim3(256), lds, fm->ctx->stream, (const TX *)dX, fm->rows, ldx, \
                           d, cd->Ct32, cd->Mp, cd->M, scale, Pa, fm->ld, a, rpb)
    if (cd->kind == RR_CENTRES_RADIAL) {
        if (x_dtype == RR_F32) { RR_CF(float, RR_CENTRES_RADIAL); }
        else { RR_CF(double, RR_CENTRES_RADIAL); }
    } else {
        if (x_dtype == RR_F32) { RR_CF(float, RR_CENTRES_SIGMOID); }
        else { RR_CF(double, RR_CENTRES_SIGMOID); }
    }
#undef RR_CF
}

}  // namespace

void rr_centres_data_free(void *p) {
    if (!p) return;
    CentresData *cd = (CentresData *)p;
    void *q[] = {cd->Ct32, cd->Ct64, cd->scale32, cd->scale64, cd->ginv32, cd->ginv64};
    for (void *x : q)
        if (x) (void)hipFree(x);
    delete cd;
}

// ---- what the resident SVI loop (rr_elbo.hip) calls: length scales in HBM, no host copy -------------------------------
// (no synchronisation in the steady state: the contraction's block partials use the context's grow-only rr_det_scratch,
// which waits for the stream once when it has to grow -- the first step, or a larger minibatch)
// RR_OK when b can be a RR_SGD_CHILD_CENTRES child of a loop on `ctx` with n_ls length scales; *M its width, *radial its kind
bool rr_centres_loop_child(const rr_basis *b, const rr_ctx *ctx, int n_ls, int *M, int *radial) {
    if (b == nullptr || b->kind != RR_KIND_CENTRES || b->centres == nullptr || b->compute != RR_F32 || b->ctx != ctx ||
        b->d > RR_CENTRES_MAX_DIM ||
        !(n_ls == 1 || n_ls == b->d))
        return false;
    const CentresData *cd = (const CentresData *)b->centres;
    *M = cd->M;
    *radial = cd->kind == RR_CENTRES_RADIAL ? 1 : 0;
    return true;
}

// What the fused small-minibatch loop (rr_svi.hip) takes of a centres handle: it computes in float64 from the handle's float64
// copy of C^T (row length *Mp), whatever the handle's own compute dtype, and needs no dimension blocking (its own limits bound d)
bool rr_centres_svi_child(const rr_basis *b, const rr_ctx *ctx, int n_ls, int *M, int *Mp, int *radial, const double **Ct64) {
    if (b == nullptr || b->kind != RR_KIND_CENTRES || b->centres == nullptr || b->ctx != ctx || !(n_ls == 1 || n_ls == b->d)) return false;
    const CentresData *cd = (const CentresData *)b->centres;
    if (cd->Ct64 == nullptr) return false;
    *M = cd->M;
    *Mp = cd->Mp;
    *radial = cd->kind == RR_CENTRES_RADIAL ? 1 : 0;
    *Ct64 = cd->Ct64;
    return true;
}

// rr_featmat_put_centres with the n_ls float64 length scales at dls (device): their float32 scales go to dscale (d floats
// the CALLER owns -- neither the handle's cache nor a centres_puts record is touched), then the feature kernel reads them
int rr_fm_put_centres_dev(rr_featmat *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, const double *dls, int n_ls,
                          float *dscale, int64_t col0) {
    CentresData *cd = centres_of(b);
    RR_REQUIRE(fm != nullptr && cd != nullptr && dls != nullptr && dscale != nullptr, "rr_fm_put_centres_dev: bad argument");
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "rr_fm_put_centres_dev: bad dtype");
    RR_REQUIRE(b->d <= RR_CENTRES_MAX_DIM && (n_ls == 1 || n_ls == b->d), "rr_fm_put_centres_dev: needs d <= %d and 1 or d length scales",
               RR_CENTRES_MAX_DIM);
    RR_REQUIRE(col0 >= 0 && col0 + (int64_t)cd->M <= fm->F, "rr_fm_put_centres_dev: columns out of range");
    RR_REQUIRE(ldx >= b->d, "rr_fm_put_centres_dev: device X needs ldx >= d = %d", b->d);
    if (fm->rows == 0) return RR_OK;
    RR_REQUIRE(dX != nullptr, "rr_fm_put_centres_dev: null X");
    RR_CHECK_HIP(hipSetDevice(fm->ctx->device));
    const int rc = rr_fm_claim(fm, col0, cd->M, "rr_fm_put_centres_dev");
    if (rc != RR_OK) return rc;
    hipLaunchKernelGGL(rr_centres_scale_dev_kernel, dim3((unsigned)((b->d + 127) / 128)), dim3(128), 0, fm->ctx->stream, dls, n_ls, b->d,
                       cd->kind == RR_CENTRES_RADIAL ? 1 : 0, dscale);
    centres_launch_features(fm, cd, b->d, dX, x_dtype, ldx, dscale, col0);
    RR_CHECK_HIP(hipGetLastError());
    return RR_OK;
}

// dS[i] += S_i, i < n_ls: the GLM step's contraction with UNIT factors -- sum E Phi (x_i - c_i)^2 (radial) or
// sum -E Phi (1 - Phi) |x_i - c_i| (sigmoid) over the matrix' rows against the EdPhi the step stored, dS in device memory;
// what is left of the gradient (1 / l^6 or 1 / l^2, the sign) is the update kernel's, from the length scales in HBM
int rr_fm_glm_centres_dev(rr_featmat *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, int64_t col0, int n_ls, double *dS) {
    CentresData *cd = centres_of(b);
    RR_REQUIRE(fm != nullptr && cd != nullptr && dS != nullptr, "rr_fm_glm_centres_dev: bad argument");
    float *U = nullptr, *err = nullptr, *m32 = nullptr;
    bool have_rows = false, have_edphi = false;
    rr_fm_pass2_views(fm->pass2, &U, &err, &m32, &have_rows, &have_edphi);
    RR_REQUIRE(have_edphi, "rr_fm_glm_centres_dev: the step did not store EdPhi");
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "rr_fm_glm_centres_dev: bad dtype");
    RR_REQUIRE(b->d <= RR_CENTRES_MAX_DIM && (n_ls == 1 || n_ls == b->d), "rr_fm_glm_centres_dev: needs d <= %d and 1 or d length scales",
               RR_CENTRES_MAX_DIM);
    RR_REQUIRE(col0 >= 0 && col0 + (int64_t)cd->M <= fm->F, "rr_fm_glm_centres_dev: columns out of range");
    RR_REQUIRE(ldx >= b->d, "rr_fm_glm_centres_dev: device X needs ldx >= d = %d", b->d);
    if (fm->rows == 0) return RR_OK;
    RR_REQUIRE(dX != nullptr, "rr_fm_glm_centres_dev: null X");
    GfacArgs gfac;
    for (int i = 0; i < 128; ++i) gfac.g[i] = 1.0;
    for (int i0 = 0; i0 < n_ls; i0 += 128) {
        const int rc = centres_contract_launch<false>(fm, cd, dX, x_dtype, ldx, col0, i0, n_ls - i0 < 128 ? n_ls - i0 : 128, gfac, dS);
        if (rc != RR_OK) return rc;
    }
    return RR_OK;
}

extern "C" {

int rr_centres_create(rr_ctx *ctx, int kind, int compute, int d, int M, const double *C, rr_basis **out) {
    RR_REQUIRE(ctx != nullptr && out != nullptr && C != nullptr, "rr_centres_create: null argument");
    *out = nullptr;
    RR_REQUIRE(kind == RR_CENTRES_RADIAL || kind == RR_CENTRES_SIGMOID, "rr_centres_create: unknown kind %d", kind);
    RR_REQUIRE(compute == RR_F32 || compute == RR_F64, "rr_centres_create: bad compute dtype %d", compute);
    RR_REQUIRE(d >= 1 && M >= 1 && (int64_t)d * M < (1 << 28), "rr_centres_create: bad shape (d=%d M=%d)", d, M);
    RR_CHECK_HIP(hipSetDevice(ctx->device));
    rr_basis *b = new rr_basis();
    CentresData *cd = new CentresData();
    b->ctx = ctx;
    b->kind = RR_KIND_CENTRES;
    b->compute = compute;
    b->d = d;
    b->n = M;
    b->centres = cd;
    cd->kind = kind;
    cd->M = M;
    cd->Mp = (M + 3) / 4 * 4;
    const size_t elems = (size_t)d * cd->Mp;
    std::vector<float> t32(elems, 0.f);
    std::vector<double> t64(elems, 0.0);
    for (int j = 0; j < M; ++j)
        for (int i = 0; i < d; ++i) {
            t64[(size_t)i * cd->Mp + j] = C[(size_t)j * d + i];
            t32[(size_t)i * cd->Mp + j] = (float)C[(size_t)j * d + i];
        }
    bool ok = hipMalloc((void **)&cd->Ct32, elems * 4) == hipSuccess && hipMalloc((void **)&cd->Ct64, elems * 8) == hipSuccess &&
              hipMalloc((void **)&cd->scale32, (size_t)d * 4) == hipSuccess && hipMalloc((void **)&cd->ginv32, (size_t)d * 4) == hipSuccess &&
              hipMalloc((void **)&cd->scale64, (size_t)d * 8) == hipSuccess && hipMalloc((void **)&cd->ginv64, (size_t)d * 8) == hipSuccess;
    ok = ok && hipMemcpy(cd->Ct32, t32.data(), elems * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(cd->Ct64, t64.data(), elems * 8, hipMemcpyHostToDevice) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        rr_set_error("rr_centres_create: device allocation or upload failed");
        rr_basis_destroy(b);
        return RR_ERR_OOM;
    }
    *out = b;
    return RR_OK;
}

int rr_centres_transform(rr_basis *b, const void *X, int x_dtype, int64_t N, int64_t ldx, const double *lenscale, int n_ls,
                         double *Phi) {
    return centres_host_call<false>(b, X, x_dtype, N, ldx, lenscale, n_ls, Phi, "rr_centres_transform");
}

int rr_centres_grad(rr_basis *b, const void *X, int x_dtype, int64_t N, int64_t ldx, const double *lenscale, int n_ls,
                    double *dPhi) {
    return centres_host_call<true>(b, X, x_dtype, N, ldx, lenscale, n_ls, dPhi, "rr_centres_grad");
}

int rr_featmat_put_centres(rr_featmat *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, const double *lenscale,
                           int n_ls, int64_t col0) {
    CentresData *cd = centres_of(b);
    RR_REQUIRE(fm != nullptr && cd != nullptr, "rr_featmat_put_centres: bad argument");
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "rr_featmat_put_centres: bad dtype");
    RR_REQUIRE(b->d <= RR_CENTRES_MAX_DIM, "rr_featmat_put_centres: needs d <= %d, got %d", RR_CENTRES_MAX_DIM, b->d);
    RR_REQUIRE(col0 >= 0 && col0 + (int64_t)cd->M <= fm->F, "rr_featmat_put_centres: columns out of range");
    RR_REQUIRE(ldx >= b->d, "rr_featmat_put_centres: device X needs ldx >= d = %d", b->d);
    int rc = centres_prepare(b, lenscale, n_ls, "rr_featmat_put_centres");
    if (rc != RR_OK || fm->rows == 0) return rc;
    RR_REQUIRE(dX != nullptr, "rr_featmat_put_centres: null X");
    RR_CHECK_HIP(hipSetDevice(fm->ctx->device));
    rc = rr_fm_claim(fm, col0, cd->M, "rr_featmat_put_centres");
    if (rc != RR_OK) return rc;
    fm->centres_puts.push_back({b, col0, std::vector<double>(lenscale, lenscale + n_ls)});  // for the contractions
    // (the P^T side copy is not written: pt_covered stays, so consumers run their transposing pass)
    centres_launch_features(fm, cd, b->d, dX, x_dtype, ldx, cd->scale32, col0);
    RR_CHECK_HIP(hipGetLastError());
    return RR_OK;
}

int rr_featmat_put_poly(rr_featmat *fm, const void *dX, int x_dtype, int64_t ldx, int d, int order, int include_bias,
                        int64_t col0) {
    RR_REQUIRE(fm != nullptr && d >= 1 && ldx >= d && order >= 0, "rr_featmat_put_poly: bad argument");
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "rr_featmat_put_poly: bad dtype");
    const int bias = include_bias ? 1 : 0;
    const int64_t w = bias + (int64_t)d * order;
    RR_REQUIRE(w >= 1 && col0 >= 0 && col0 + w <= fm->F, "rr_featmat_put_poly: columns out of range");
    if (fm->rows == 0) return RR_OK;
    RR_REQUIRE(dX != nullptr, "rr_featmat_put_poly: null X");
    RR_CHECK_HIP(hipSetDevice(fm->ctx->device));
    const int rc = rr_fm_claim(fm, col0, w, "rr_featmat_put_poly");
    if (rc != RR_OK) return rc;
    const dim3 grid((unsigned)((fm->rows * d + 255) / 256));
    if (x_dtype == RR_F32)
        hipLaunchKernelGGL(rr_poly_features_kernel<float>, grid, dim3(256), 0, fm->ctx->stream, (const float *)dX, fm->rows, ldx, d,
                           order, bias, fm->P + col0, fm->ld);
    else
        hipLaunchKernelGGL(rr_poly_features_kernel<double>, grid, dim3(256), 0, fm->ctx->stream, (const double *)dX, fm->rows, ldx,
                           d, order, bias, fm->P + col0, fm->ld);
    RR_CHECK_HIP(hipGetLastError());
    return RR_OK;
}

int rr_featmat_pass2_centres(rr_featmat *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, int64_t col0, double *dg) {
    return centres_contract<true>(fm, b, dX, x_dtype, ldx, col0, dg, "rr_featmat_pass2_centres");
}

int rr_featmat_glm_centres(rr_featmat *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, int64_t col0, double *dg) {
    return centres_contract<false>(fm, b, dX, x_dtype, ldx, col0, dg, "rr_featmat_glm_centres");
}

// ---- the float64 feature matrix' entry points (struct rr_featmat64: rr_internal.h) -----------------------------------------

int rr_featmat64_put_centres(rr_featmat64 *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, const double *lenscale,
                             int n_ls, int64_t col0) {
    CentresData *cd = centres_of(b);
    RR_REQUIRE(fm != nullptr && cd != nullptr, "rr_featmat64_put_centres: bad argument");
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "rr_featmat64_put_centres: bad dtype");
    RR_REQUIRE(b->d <= RR_CENTRES_MAX_DIM, "rr_featmat64_put_centres: needs d <= %d, got %d", RR_CENTRES_MAX_DIM, b->d);
    RR_REQUIRE(col0 >= 0 && col0 + (int64_t)cd->M <= fm->F, "rr_featmat64_put_centres: columns out of range");
    RR_REQUIRE(ldx >= b->d, "rr_featmat64_put_centres: device X needs ldx >= d = %d", b->d);
    int rc = centres_prepare(b, lenscale, n_ls, "rr_featmat64_put_centres");
    if (rc != RR_OK || fm->rows == 0) return rc;
    RR_REQUIRE(dX != nullptr, "rr_featmat64_put_centres: null X");
    RR_CHECK_HIP(hipSetDevice(fm->ctx->device));
    rc = rr_fm64_claim(fm, col0, cd->M, "rr_featmat64_put_centres");
    if (rc != RR_OK) return rc;
    fm->centres_puts.push_back({b, col0, std::vector<double>(lenscale, lenscale + n_ls)});  // for rr_featmat64_pass2_centres
    const int d = b->d;
    const int a = (int)(col0 & 1);
    const int rpb = 256;
    const dim3 grid((unsigned)((fm->rows + rpb - 1) / rpb), (unsigned)((a + cd->M + CT64 - 1) / CT64));
    const bool wide = d > DB;  // dimension blocks; the LDS of d = DB
    const int dl = wide ? DB : d;
    const size_t lds = ((size_t)dl * CT64 + (size_t)((dl + 1) & ~1) + (size_t)RT64 * (dl + 1)) * 8;
    double *Pa = fm->P + (col0 - a);
    const int64_t cmax = fm->ld - (col0 - a);
#define RR_CF64(TX, KIND)                                                                                                        \
    if (wide)                                                                                                                    \
        hipLaunchKernelGGL((rr_centres_features64_wide_kernel<TX, KIND>), grid, dim3(256), lds, fm->ctx->stream, (const TX *)dX,  \
                           fm->rows, ldx, d, cd->Ct64, cd->Mp, cd->M, cd->scale64, Pa, fm->ld, a, rpb, cmax);                     \
    else                                                                                                                         \
        hipLaunchKernelGGL((rr_centres_features64_kernel<TX, KIND>), grid, dim3(256), lds, fm->ctx->stream, (const TX *)dX, fm->rows, \
                           ldx, d, cd->Ct64, cd->Mp, cd->M, cd->scale64, Pa, fm->ld, a, rpb, cmax)
    if (cd->kind == RR_CENTRES_RADIAL) {
        if (x_dtype == RR_F32) { RR_CF64(float, RR_CENTRES_RADIAL); }
        else { RR_CF64(double, RR_CENTRES_RADIAL); }
    } else {
        if (x_dtype == RR_F32) { RR_CF64(float, RR_CENTRES_SIGMOID); }
        else { RR_CF64(double, RR_CENTRES_SIGMOID); }
    }
#undef RR_CF64
    RR_CHECK_HIP(hipGetLastError());
    return RR_OK;
}

int rr_featmat64_put_poly(rr_featmat64 *fm, const void *dX, int x_dtype, int64_t ldx, int d, int order, int include_bias,
                          int64_t col0) {
    RR_REQUIRE(fm != nullptr && d >= 1 && ldx >= d && order >= 0, "rr_featmat64_put_poly: bad argument");
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "rr_featmat64_put_poly: bad dtype");
    const int bias = include_bias ? 1 : 0;
    const int64_t w = bias + (int64_t)d * order;
    RR_REQUIRE(w >= 1 && col0 >= 0 && col0 + w <= fm->F, "rr_featmat64_put_poly: columns out of range");
    if (fm->rows == 0) return RR_OK;
    RR_REQUIRE(dX != nullptr, "rr_featmat64_put_poly: null X");
    RR_CHECK_HIP(hipSetDevice(fm->ctx->device));
    const int rc = rr_fm64_claim(fm, col0, w, "rr_featmat64_put_poly");
    if (rc != RR_OK) return rc;
    const dim3 grid((unsigned)((fm->rows * d + 255) / 256));
    if (x_dtype == RR_F32)
        hipLaunchKernelGGL(rr_poly_features64_kernel<float>, grid, dim3(256), 0, fm->ctx->stream, (const float *)dX, fm->rows, ldx, d,
                           order, bias, fm->P + col0, fm->ld);
    else
        hipLaunchKernelGGL(rr_poly_features64_kernel<double>, grid, dim3(256), 0, fm->ctx->stream, (const double *)dX, fm->rows, ldx,
                           d, order, bias, fm->P + col0, fm->ld);
    RR_CHECK_HIP(hipGetLastError());
    return RR_OK;
}

extern "C++" {
// SLM: the second pass' E = Err m^T - Phi C (after rr_featmat64_pass2_rows); else the GLM step's E = EdPhi (after a step that
// stored it, rr_glm64.hip) -- one launcher, as centres_contract<SLM> is for the f32 matrix
template <bool SLM>
static int centres_contract64(rr_featmat64 *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, int64_t col0, double *dg,
                              const char *who) {
    CentresData *cd = centres_of(b);
    RR_REQUIRE(fm != nullptr && cd != nullptr && dg != nullptr, "%s: bad argument", who);
    if (SLM) RR_REQUIRE(fm->Pt != nullptr && fm->have_rows, "%s: call rr_featmat64_pass2_rows first", who);
    else RR_REQUIRE(fm->U != nullptr && fm->have_edphi, "%s: call rr_featmat64_glm_step first", who);
    RR_REQUIRE(x_dtype == RR_F32 || x_dtype == RR_F64, "%s: bad dtype", who);
    RR_REQUIRE(b->d <= RR_CENTRES_MAX_DIM, "%s: needs d <= %d, got %d", who, RR_CENTRES_MAX_DIM, b->d);
    RR_REQUIRE(col0 >= 0 && col0 + (int64_t)cd->M <= fm->F, "%s: columns out of range", who);
    RR_REQUIRE(ldx >= b->d, "%s: device X needs ldx >= d = %d", who, b->d);
    const std::vector<double> *put_ls = nullptr;
    for (const auto &pc : fm->centres_puts)
        if (pc.basis == b && pc.col0 == col0) put_ls = &pc.ls;
    RR_REQUIRE(put_ls != nullptr, "%s: this basis was not put at column %lld since rr_featmat64_begin (rr_featmat64_put_centres)", who,
               (long long)col0);
    if (fm->rows == 0) return RR_OK;
    RR_REQUIRE(dX != nullptr, "%s: null X", who);
    const int nls = (int)put_ls->size();
    RR_REQUIRE(nls == 1 || nls == b->d, "%s: the block was put with %d length scales, d = %d", who, nls, b->d);
    rr_ctx *c = fm->ctx;
    RR_CHECK_HIP(hipSetDevice(c->device));
    const int ctiles = (cd->M + CT64 - 1) / CT64;
    // about 8 workgroups per compute unit, whole sub-tiles of rows each: few enough partial sums for the second stage
    int64_t rpb = (fm->rows * ctiles + (int64_t)c->num_cu * 8 - 1) / ((int64_t)c->num_cu * 8);
    rpb = (rpb + RT64 - 1) / RT64 * RT64;
    const dim3 grid((unsigned)((fm->rows + rpb - 1) / rpb), (unsigned)ctiles);
    const int64_t nblocks = (int64_t)grid.x * grid.y;
    const double *P = fm->P + col0, *Uc = fm->U + col0, *mv = fm->m + col0;
    // one launch and one second stage per block of 128 length scales (centres_contract_launch's pattern): the kernel sees
    // columns i0 .. of X and rows i0 .. of C^T as its dimensions 0 .. nd - 1
    for (int i0 = 0; i0 < nls; i0 += 128) {
        const int nd = nls - i0 < 128 ? nls - i0 : 128;
        GfacArgs gfac;
        centres_gfac(cd, *put_ls, i0, &gfac);
        int DP = 1;
        while (DP < nd) DP *= 2;
        void *part = nullptr;
        int rc = rr_det_scratch(c, (size_t)nblocks * nd * 8, &part);
        if (rc != RR_OK) return rc;
        const size_t lds = ((size_t)2 * 16 * DP + (size_t)RT64 * CT64 + (size_t)RT64 * (DP + 1) + 256) * 8;
        const double *Ct = cd->Ct64 + (size_t)i0 * cd->Mp;
#define RR_CC64(TX, KIND)                                                                                                      \
        hipLaunchKernelGGL((rr_centres_contract64_kernel<TX, KIND, SLM>), grid, dim3(256), lds, c->stream, (const TX *)dX + i0, fm->rows, ldx, \
                           nd, DP, Ct, cd->Mp, cd->M, P, Uc, fm->ld, fm->err, mv, gfac, (int)rpb, (double *)part)
        if (cd->kind == RR_CENTRES_RADIAL) {
            if (x_dtype == RR_F32) RR_CC64(float, RR_CENTRES_RADIAL);
            else RR_CC64(double, RR_CENTRES_RADIAL);
        } else {
            if (x_dtype == RR_F32) RR_CC64(float, RR_CENTRES_SIGMOID);
            else RR_CC64(double, RR_CENTRES_SIGMOID);
        }
#undef RR_CC64
        RR_CHECK_HIP(hipGetLastError());
        rc = rr_det_reduce(c, (const double *)part, nblocks, nd, nd, dg + i0);
        if (rc != RR_OK) return rc;
    }
    return RR_OK;
}
}  // extern "C++"

int rr_featmat64_pass2_centres(rr_featmat64 *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, int64_t col0, double *dg) {
    return centres_contract64<true>(fm, b, dX, x_dtype, ldx, col0, dg, "rr_featmat64_pass2_centres");
}

int rr_featmat64_glm_centres(rr_featmat64 *fm, rr_basis *b, const void *dX, int x_dtype, int64_t ldx, int64_t col0, double *dg) {
    return centres_contract64<false>(fm, b, dX, x_dtype, ldx, col0, dg, "rr_featmat64_glm_centres");
}

int rr_featmat64_download(rr_featmat64 *fm, double *out) {
    RR_REQUIRE(fm != nullptr && (out != nullptr || fm->rows == 0), "rr_featmat64_download: null argument");
    if (fm->rows == 0) return RR_OK;
    RR_CHECK_HIP(hipSetDevice(fm->ctx->device));
    RR_CHECK_HIP(hipMemcpyAsync(out, fm->P, (size_t)fm->rows * fm->ld * sizeof(double), hipMemcpyDeviceToHost, fm->ctx->stream));
    RR_CHECK_HIP(hipStreamSynchronize(fm->ctx->stream));
    return RR_OK;
}

}  // extern "C"
