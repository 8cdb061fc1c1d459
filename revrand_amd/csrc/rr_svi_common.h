// What the small-minibatch SVI loops (rr_svi.hip: one persistent kernel; rr_svi_wide.hip: a chain of kernels per step) and the
// resident step of rr_elbo.hip share: the counter-based sampler, the likelihood terms, the updater -- pinned bit for bit by
// tests/test_gpu_sampler_exact.py and tests/test_gpu_lik_tails.py, so they exist ONCE -- and the host side of a loop handle's
// coordinate state.  Include after rr_internal.h (the RR_BOUNDS guards of hipMalloc / hipFree and RR_DEV_ASSERT apply here).
#pragma once

#include <cmath>

// ---- the sampler: the normal for (seed, step, counter) is two SplitMix64 rounds + Box-Muller -------------------------------
__host__ __device__ __forceinline__ uint64_t rr_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the key of step `step` (key0 + t; a random start: key0 + candidate) of the stream `seed`
__host__ __device__ __forceinline__ uint64_t rr_svi_stepkey(uint64_t seed, uint64_t step) {
    return rr_splitmix64(seed ^ (step * 0xD1B54A32D192ED03ull));
}

// Adam's 1 - beta1^t, 1 - beta2^t of step t = 1, 2, ... (sgd.py:322-323): formed on the host, no pow on the device
static inline void rr_svi_adam_bias(const double up[4], int64_t t, double &b1t, double &b2t) {
    const double tt = (double)t;
    b1t = 1.0 - pow(up[1], tt);
    b2t = 1.0 - pow(up[2], tt);
}

#ifdef __HIPCC__
// the draw for (stepkey, counter): a float32 expression, the same in rr_glm_draw_kernel and in both loops
__device__ __forceinline__ float rr_svi_draw(uint64_t stepkey, uint64_t ctr) {
    const uint64_t h = rr_splitmix64(stepkey ^ ctr);
    const float u1 = ((float)(uint32_t)(h >> 40) + 1.0f) * (1.0f / 16777216.0f);  // (0, 1]
    const float u2 = (float)(uint32_t)((h >> 8) & 0xFFFFFFu) * (1.0f / 16777216.0f);
    return sqrtf(-2.0f * __logf(u1)) * __builtin_amdgcn_cosf(u2);  // cos of u2 revolutions
}

// ---- the likelihood terms in float64 ---------------------------------------------------------------------------------------
__device__ __forceinline__ double rr_svi_softplus(double f) { return fmax(f, 0.0) + log1p(exp(-fabs(f))); }
__device__ __forceinline__ double rr_svi_expit(double f) {
    const double e = exp(-fabs(f));
    return f >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e);
}

// d loglike / d f and the f-dependent part of loglike (Gaussian: the squared error)   likelihoods.py:46-104,171-233,298-368,456-521
__device__ __forceinline__ void rr_svi_lik(int lik, double f, double y, double n, double ivar, double &df, double &ll) {
    if (lik == RR_LIK_BERNOULLI) {
        df = y - rr_svi_expit(f);
        ll = y * f - rr_svi_softplus(f);
    } else if (lik == RR_LIK_BINOMIAL) {
        df = y - n * rr_svi_expit(f);
        ll = y * f - n * rr_svi_softplus(f);
    } else if (lik == RR_LIK_GAUSSIAN) {
        const double er = y - f;
        df = er * ivar;
        ll = er * er;
    } else if (lik == RR_LIK_POISSON_EXP) {
        const double g = exp(f);
        df = y - g;
        ll = y * f - g;
    } else {
        const double g = fmax(rr_svi_softplus(f), 1e-100);
        df = rr_svi_expit(f) * (y / g - 1.0);
        ll = y * log(g) - g;
    }
}

typedef __attribute__((address_space(3))) double ldsd;   // LDS pointers keep their address space: ds_read / ds_write, never flat
typedef __attribute__((address_space(3))) float ldsf;
typedef __attribute__((address_space(3))) unsigned char ldsb;

__device__ __forceinline__ double rr_svi_wave_sum(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// entry (row, i) of a child's resident X (C: SviChild / SwChild)
template <typename C>
__device__ __forceinline__ double rr_svi_xval(const C &c, int64_t row, int i) {
    return c.x_f64 ? ((const double *)c.X)[row * c.ldx + i] : (double)((const float *)c.X)[row * c.ldx + i];
}

// one coordinate's truncation + updater + clip (sgd.py:404-420, :14-330); g is the gradient in z space (A: updater, up[4]);
// s1, s2: the updater's state (Adadelta: E[g^2], E[dx^2]; AdaGrad: sum g^2; momentum: dx; Adam: m, v), b1t, b2t: rr_svi_adam_bias
template <typename A>
__device__ __forceinline__ double rr_svi_update(const A &a, double zz, double g, double lo, double hi, double &s1, double &s2,
                                                double b1t, double b2t) {
#pragma clang fp contract(off)
    if (zz <= lo) g = (g <= 0.0 || g != g) ? g : 0.0;  // np.minimum(grad, 0) on a coordinate sitting on its lower bound
    if (zz >= hi) g = (g >= 0.0 || g != g) ? g : 0.0;
    double zn;
    switch (a.updater) {
        case RR_UPD_SGD: zn = zz - a.up[0] * g; break;
        case RR_UPD_ADADELTA: {  // up = (rho, epsilon)
            const double eg2 = a.up[0] * s1 + (1 - a.up[0]) * (g * g);
            const double dx = -g * sqrt(s2 + a.up[1]) / sqrt(eg2 + a.up[1]);
            s1 = eg2;
            s2 = a.up[0] * s2 + (1 - a.up[0]) * (dx * dx);
            zn = zz + dx;
        } break;
        case RR_UPD_ADAGRAD: {  // up = (eta, epsilon)
            const double h = s1 + g * g;
            s1 = h;
            zn = zz - a.up[0] * g / (a.up[1] + sqrt(h));
        } break;
        case RR_UPD_MOMENTUM: {  // up = (rho, eta)
            const double dx = a.up[0] * s1 - a.up[1] * g;
            s1 = dx;
            zn = zz + dx;
        } break;
        default: {  // Adam: up = (alpha, beta1, beta2, epsilon)
            const double m = a.up[1] * s1 + (1 - a.up[1]) * g;
            const double v = a.up[2] * s2 + (1 - a.up[2]) * (g * g);
            s1 = m;
            s2 = v;
            zn = zz - a.up[0] * (m / b1t) / (sqrt(v / b2t) + a.up[3]);
        }
    }
    return zn < lo ? lo : (zn > hi ? hi : zn);
}

// log z_l = logsumexp_j log N_jl, log N_jl = -(F log 2 pi + q_jl) / 2, from the full q (K, K), by threads l < K (Q, Z: LDS or
// HBM pointers); no barrier behind it: the caller places its own   glm.py:221-222
template <typename Q, typename Z>
__device__ __forceinline__ void rr_svi_logz(int F, int K, Q q, Z logz) {
    const int tid = threadIdx.x;
    if (tid < K) {
        double mx = -INFINITY;
        for (int j = 0; j < K; ++j) mx = fmax(mx, -0.5 * ((double)F * 1.8378770664093453 + q[j * K + tid]));
        double sm = 0.0;
        for (int j = 0; j < K; ++j) sm += exp(-0.5 * ((double)F * 1.8378770664093453 + q[j * K + tid]) - mx);
        logz[tid] = log(sm) + mx;
    }
}
#endif

// ---- the host side of a loop handle ----------------------------------------------------------------------------------------
// The np coordinates in z space with the updater's state, bounds and log flags, the per-step records, the step count, and the
// grow-only buffers of the random starts.  All device memory; both handles embed one.
struct RrSviState {
    double *z = nullptr, *s1 = nullptr, *s2 = nullptr, *lower = nullptr, *upper = nullptr, *objs = nullptr, *norms = nullptr;
    unsigned char *islog = nullptr;
    int64_t np = 0, maxiter = 0, t = 0;
    double *cand = nullptr, *out = nullptr;  // rr_svi_state_candidates
    size_t cand_cap = 0;                     // candidates both hold
};

// allocate, upload the start, zero the updater's state and the records (the first error, or hipSuccess; rr_svi_state_free cleans up)
static hipError_t rr_svi_state_alloc(RrSviState &st, int64_t np, int64_t maxiter, const double *z0, const double *lower,
                                     const double *upper, const unsigned char *is_log) {
    st.np = np;
    st.maxiter = maxiter;
    const size_t nb = (size_t)np * 8, nr = (size_t)maxiter * 8;
    hipError_t e = hipMalloc((void **)&st.z, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&st.s1, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&st.s2, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&st.lower, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&st.upper, nb);
    if (e == hipSuccess) e = hipMalloc((void **)&st.islog, (size_t)np);
    if (e == hipSuccess) e = hipMalloc((void **)&st.objs, nr);
    if (e == hipSuccess) e = hipMalloc((void **)&st.norms, nr);
    if (e == hipSuccess) e = hipMemcpy(st.z, z0, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(st.lower, lower, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(st.upper, upper, nb, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(st.islog, is_log, (size_t)np, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(st.s1, 0, nb);
    if (e == hipSuccess) e = hipMemset(st.s2, 0, nb);
    if (e == hipSuccess) e = hipMemset(st.objs, 0, nr);
    if (e == hipSuccess) e = hipMemset(st.norms, 0, nr);
    return e;
}

static void rr_svi_state_free(RrSviState &st) {
    void *q[] = {st.z, st.s1, st.s2, st.lower, st.upper, st.islog, st.objs, st.norms, st.cand, st.out};
    for (void *v : q)
        if (v) (void)hipFree(v);
    st = RrSviState();
}

// a new start (any of the four may be null: kept), before the first step; the caller has checked t == 0
static int rr_svi_state_set_start(RrSviState &st, rr_ctx *c, const double *z0, const double *lower, const double *upper,
                                  const unsigned char *is_log) {
    RR_CHECK_HIP(hipSetDevice(c->device));
    RR_CHECK_HIP(hipStreamSynchronize(c->stream));
    const size_t nb = (size_t)st.np * 8;
    if (z0) RR_CHECK_HIP(hipMemcpy(st.z, z0, nb, hipMemcpyHostToDevice));
    if (lower) RR_CHECK_HIP(hipMemcpy(st.lower, lower, nb, hipMemcpyHostToDevice));
    if (upper) RR_CHECK_HIP(hipMemcpy(st.upper, upper, nb, hipMemcpyHostToDevice));
    if (is_log) RR_CHECK_HIP(hipMemcpy(st.islog, is_log, (size_t)st.np, hipMemcpyHostToDevice));
    return RR_OK;
}

// z and the records of the t steps done (any of the four may be null), after the stream has drained
static int rr_svi_state_read(RrSviState &st, rr_ctx *c, double *z, double *objs, double *norms, int64_t *steps) {
    RR_CHECK_HIP(hipSetDevice(c->device));
    RR_CHECK_HIP(hipStreamSynchronize(c->stream));
    if (z) RR_CHECK_HIP(hipMemcpy(z, st.z, (size_t)st.np * 8, hipMemcpyDeviceToHost));
    if (objs && st.t) RR_CHECK_HIP(hipMemcpy(objs, st.objs, (size_t)st.t * 8, hipMemcpyDeviceToHost));
    if (norms && st.t) RR_CHECK_HIP(hipMemcpy(norms, st.norms, (size_t)st.t * 8, hipMemcpyDeviceToHost));
    if (steps) *steps = st.t;
    return RR_OK;
}

// cand (ncand, np) and out (ncand) of the random starts: grow-only, the candidates queued for upload on the context's stream
static int rr_svi_state_candidates(RrSviState &st, rr_ctx *c, int ncand, const double *cand_host) {
    if (st.cand_cap < (size_t)ncand) {
        RR_CHECK_HIP(hipStreamSynchronize(c->stream));
        if (st.cand) (void)hipFree(st.cand);
        if (st.out) (void)hipFree(st.out);
        st.cand = st.out = nullptr;
        st.cand_cap = 0;
        RR_CHECK_HIP(hipMalloc((void **)&st.cand, (size_t)ncand * st.np * 8));
        RR_CHECK_HIP(hipMalloc((void **)&st.out, (size_t)ncand * 8));
        st.cand_cap = (size_t)ncand;
    }
    RR_CHECK_HIP(hipMemcpyAsync(st.cand, cand_host, (size_t)ncand * st.np * 8, hipMemcpyHostToDevice, c->stream));
    return RR_OK;
}

// the argument checks rr_glm_svi_create* and rr_glm_sviw*_create open with, in their order; clears *out after the first
static int rr_svi_check_create(const char *who, int maxchild, int maxk, const rr_ctx *ctx, int n_children, const rr_glm_sgd_child *children,
                               const void *const *dX, const int *x_dtype, const int64_t *ldx, int64_t N, const void *dy,
                               const void *drowarg, int dtype, int K, int L, int M, int lik, int n_lik, const double *z0,
                               const double *lower, const double *upper, const unsigned char *is_log, int updater,
                               const double *upd_par, int64_t maxiter, void **out) {
    RR_REQUIRE(ctx != nullptr && children != nullptr && dX != nullptr && x_dtype != nullptr && ldx != nullptr && dy != nullptr &&
               z0 != nullptr && lower != nullptr && upper != nullptr && is_log != nullptr && upd_par != nullptr && out != nullptr,
               "%s: null argument", who);
    *out = nullptr;
    RR_REQUIRE(n_children >= 1 && n_children <= maxchild, "%s: 1 <= children <= %d", who, maxchild);
    RR_REQUIRE(K >= 1 && K <= maxk && L >= 1 && M >= 1 && N >= 1, "%s: bad K, L, minibatch or N", who);
    RR_REQUIRE(lik >= RR_LIK_BERNOULLI && lik <= RR_LIK_POISSON_SOFTPLUS && (lik == RR_LIK_GAUSSIAN) == (n_lik == 1),
               "%s: likelihood %d with %d likelihood parameter(s)", who, lik, n_lik);
    RR_REQUIRE((lik == RR_LIK_BINOMIAL) == (drowarg != nullptr), "%s: the per-row argument goes with the binomial likelihood", who);
    RR_REQUIRE(updater >= RR_UPD_SGD && updater <= RR_UPD_ADAM, "%s: unknown updater %d", who, updater);
    RR_REQUIRE(maxiter >= 1 && maxiter < ((int64_t)1 << 31) && N < ((int64_t)1 << 31), "%s: bad maxiter / N", who);
    RR_REQUIRE(dtype == RR_F32 || dtype == RR_F64, "%s: bad dtype", who);
    return RR_OK;
}

// a random Fourier or spectral-mixture child's W (d, n) as given, on the device; null (the HIP error cleared) when that fails
static double *rr_svi_upload_w(const rr_basis *b) {
    double *w = nullptr;
    if (hipMalloc((void **)&w, b->W.size() * 8) != hipSuccess ||
        hipMemcpy(w, b->W.data(), b->W.size() * 8, hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipGetLastError();
        if (w) (void)hipFree(w);
        return nullptr;
    }
    return w;
}
