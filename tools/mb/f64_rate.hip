// Micro-benchmark (run on the GPU box): the rate of separately rounded double multiply-add pairs out of registers -- what the Gram
// kernel of ensemble_modes.hip could reach if nothing but its v_mul_f64 / v_add_f64 stream cost anything.
//   hipcc -O3 --offload-arch=gfx950 tools/mb/f64_rate.hip -o tools/mb/f64_rate
// Every lane holds an 8 x 8 tile of accumulators and two vectors of 8 doubles, as a lane of the pair kernel does, and adds the 64
// rounded products again and again: acc[i][j] = acc[i][j] + a[i] * b[j], contraction off, so one v_mul_f64 and one v_add_f64 a pair.
// No memory traffic in the loop.  Prints one JSON line: the median [min - max] of 5 timed launches in pairs per second.
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e_), __LINE__); return 1; } } while (0)

#pragma clang fp contract(off)

__global__ __launch_bounds__(64) void k_pairs(double* out, int iters, double seed) {
    double acc[64], a[8], b[8];
    for (int i = 0; i < 8; ++i) { a[i] = seed + 1e-3 * (threadIdx.x + i); b[i] = seed - 1e-3 * (blockIdx.x % 7 + i); }
    for (int t = 0; t < 64; ++t) acc[t] = 0.0;
    for (int it = 0; it < iters; ++it) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[i * 8 + j] = acc[i * 8 + j] + a[i] * b[j];
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) asm volatile("" : "+v"(a[i]));      // (keeps the products from being hoisted out of the loop)
    }
    double s = 0.0;
    for (int t = 0; t < 64; ++t) s = s + acc[t];
    if (s == 12345.678) out[0] = s;
}

int main() {
    double* out;
    CK(hipMalloc(&out, 256));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int iters = 4096, waves_per_cu = 8, grid = prop.multiProcessorCount * waves_per_cu;
    double rate[5];
    for (int r = -2; r < 5; ++r) {
        CK(hipEventRecord(e0));
        hipLaunchKernelGGL(k_pairs, dim3(grid), dim3(64), 0, 0, out, iters, 0.5);
        CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
        float ms;
        CK(hipEventElapsedTime(&ms, e0, e1));
        if (r >= 0) rate[r] = (double)grid * 64.0 * iters * 64.0 / (ms * 1e-3);
    }
    std::sort(rate, rate + 5);
    printf("{\"tool\": \"tools/mb/f64_rate.hip\", \"device\": \"%s\", \"compute_units\": %d, \"waves_per_cu\": %d, \"pairs_per_s\": {\"median\": %.4g, \"min\": %.4g, \"max\": %.4g}}\n",
           prop.name, prop.multiProcessorCount, waves_per_cu, rate[2], rate[0], rate[4]);
    return 0;
}
