// How accurate are the hardware v_sin_f32 / v_cos_f32 (argument in revolutions) on [-1/2, 1/2]?  (The f32 FastFood chain
// kernels reduce their phase to that interval and call exactly these two; tests/test_gpu_fastfood_exact.py takes its
// float32 feature bound from the figure printed here, docs/KERNELS.md 3.7.)
//   hipcc --offload-arch=gfx950 -O3 tools/probes/sincos_probe.hip -o /tmp/sincos_probe && /tmp/sincos_probe
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdio>
#include <vector>

// every multiple of 2^-16 in [-1/2, 1/2]: t = (i - 32768) 2^-16, i = 0 .. 65536
__global__ void __launch_bounds__(256) sincos_rev(float *s, float *c, int n) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float t = (float)(i - 32768) * 0x1p-16f;
    s[i] = __builtin_amdgcn_sinf(t);
    c[i] = __builtin_amdgcn_cosf(t);
}

// the same instructions at t + m, m whole revolutions (t + m is exact in float32 for multiples of 2^-4 below 2^20): does the
// instruction reduce a large argument itself, i.e. does the kernels' own t - rint(t) change anything?
__global__ void __launch_bounds__(64) sincos_far(float *s, float *c, float m) {
    const float t = (float)((int)threadIdx.x - 8) * 0x1p-4f;  // threads 0 .. 16: t = -1/2 .. 1/2 in steps of 1/16
    s[threadIdx.x] = __builtin_amdgcn_sinf(t + m);
    c[threadIdx.x] = __builtin_amdgcn_cosf(t + m);
}

int main() {
    const int n = 65537;
    float *ds, *dc;
    if (hipMalloc(&ds, n * 4) != hipSuccess || hipMalloc(&dc, n * 4) != hipSuccess) { printf("alloc failed\n"); return 1; }
    hipLaunchKernelGGL(sincos_rev, dim3((n + 255) / 256), dim3(256), 0, 0, ds, dc, n);
    if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
    std::vector<float> s(n), c(n);
    if (hipMemcpy(s.data(), ds, n * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(c.data(), dc, n * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
    const long double two_pi = 6.283185307179586476925286766559L;
    double es = 0, ec = 0, ts = 0, tc = 0;
    for (int i = 0; i < n; ++i) {
        const double t = (double)(i - 32768) / 65536.0;
        const double e1 = fabs((double)s[i] - (double)sinl(two_pi * t)), e2 = fabs((double)c[i] - (double)cosl(two_pi * t));
        if (e1 > es) { es = e1; ts = t; }
        if (e2 > ec) { ec = e2; tc = t; }
    }
    printf("v_sin_f32 max |error| %.6e at t = %.10f rev (%.3f x 2^-24)\n", es, ts, es * 16777216.0);
    printf("v_cos_f32 max |error| %.6e at t = %.10f rev (%.3f x 2^-24)\n", ec, tc, ec * 16777216.0);
    printf("SINCOS_F32_MAX_ERR %.6e\n", es > ec ? es : ec);
    const float far[] = {0.f, 255.f, 257.f, 1024.f, 65536.f, 524288.f};
    for (float m : far) {
        hipLaunchKernelGGL(sincos_far, dim3(1), dim3(64), 0, 0, ds, dc, m);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) { printf("launch failed\n"); return 1; }
        if (hipMemcpy(s.data(), ds, 17 * 4, hipMemcpyDeviceToHost) != hipSuccess ||
            hipMemcpy(c.data(), dc, 17 * 4, hipMemcpyDeviceToHost) != hipSuccess) { printf("copy failed\n"); return 1; }
        double e = 0;
        for (int i = 0; i < 17; ++i) {
            const double t = (i - 8) / 16.0;
            e = fmax(e, fmax(fabs((double)s[i] - (double)sinl(two_pi * t)), fabs((double)c[i] - (double)cosl(two_pi * t))));
        }
        printf("at t + %.0f revolutions (t multiples of 1/16): max |error| %.3e\n", (double)m, e);
    }
    return 0;
}
