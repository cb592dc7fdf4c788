// HBM-bound streams over the members of an ensemble of stochastic samples.
//
//   ensemble_reduce_kernel : mean and unbiased std over the members of an ensemble of stochastic samples
//   ensemble_broadcast_kernel : the condition image of an ensemble pass's virtual samples
//   ensemble_quantiles_kernel : per-pixel quantiles over the members
#include "midd_internal.h"
#include "quantile_common.h"
#include <initializer_list>

namespace midd {

// ------------------------------------------------------------------------------ ensembles of stochastic samples
// samples [B][K][chw] -> mean [B][chw], unbiased std [B][chw] over the K members of every pixel.  A thread owns V
// neighbouring pixels (V = 4: one 16-byte load per member, 1 KiB per wave instruction, when chw is a multiple of 4 and the
// pointers are 16-byte aligned; V = 1 otherwise) and walks the K member planes chw floats apart, twice (sum; deviations from
// the mean), one load in flight per walk step.  The algorithm needs (K + 2) * 4 bytes per pixel; what the kernel reaches
// against them, at a cache-resident and at a 512 MiB shape, is measured by tools/ensemble_ab.py.
// THE ARITHMETIC IS FIXED (include/midd.h: mi_ensemble_reduce) and per pixel, so neither V nor the grid shows
// in the result: double precision, members in index order, every operation rounded to nearest on its own (add_rn64, sub_rn64,
// mul_rn64: pointwise_common.h).
template <int V>
__global__ __launch_bounds__(256)
void ensemble_reduce_kernel(const float* __restrict__ samples, int K, unsigned long long chw, float* __restrict__ mean, float* __restrict__ stdv) {
    const unsigned long long e = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (e >= chw) return;                                   // (V == 4: chw % 4 == 0, so e + 3 < chw)
    const size_t b = blockIdx.y;
    const float* src = samples + b * (size_t)K * chw + e;
    float x[V];
    auto load = [&](int m) {
        if constexpr (V == 4) { const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)m * chw); x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
        else x[0] = src[(size_t)m * chw];
    };
    double sum[V], m64[V];
#pragma unroll
    for (int j = 0; j < V; ++j) sum[j] = 0.0;
    for (int m = 0; m < K; ++m) {
        load(m);
#pragma unroll
        for (int j = 0; j < V; ++j) sum[j] = add_rn64(sum[j], (double)x[j]);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) m64[j] = __ddiv_rn(sum[j], (double)K);
    float out[V];
    if (mean) {
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = __double2float_rn(m64[j]);
        if constexpr (V == 4) *reinterpret_cast<f32x4*>(mean + b * chw + e) = (f32x4){out[0], out[1], out[2], out[3]};
        else mean[b * chw + e] = out[0];
    }
    if (stdv) {
        double q[V];
#pragma unroll
        for (int j = 0; j < V; ++j) q[j] = 0.0;
        for (int m = 0; m < K; ++m) {
            load(m);
#pragma unroll
            for (int j = 0; j < V; ++j) { const double d = sub_rn64((double)x[j], m64[j]); q[j] = add_rn64(q[j], mul_rn64(d, d)); }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = __double2float_rn(__dsqrt_rn(__ddiv_rn(q[j], (double)(K - 1))));
        if constexpr (V == 4) *reinterpret_cast<f32x4*>(stdv + b * chw + e) = (f32x4){out[0], out[1], out[2], out[3]};
        else stdv[b * chw + e] = out[0];
    }
}

// V = 4?  When chw is a multiple of 4 and every pointer of the list is 16-byte aligned (a null one is).  grid (chunks of 256 * V
// elements, rows)
static bool ensemble_v4(unsigned long long chw, std::initializer_list<const void*> ptrs, int rows, dim3* grid) {
    bool v4 = chw % 4 == 0;
    for (const void* p : ptrs) v4 = v4 && aligned16(p);
    *grid = dim3((unsigned)(((v4 ? chw / 4 : chw) + 255) / 256), rows);
    return v4;
}

hipError_t ensemble_reduce_launch(const float* samples, int B, int K, unsigned long long chw, float* mean, float* stdv, hipStream_t s) {
    if (B < 1 || B > 65535 || K < 1 || chw < 1 || chw >= (1ull << 32) || (!mean && !stdv) || (stdv && K < 2)) return hipErrorInvalidValue;
    dim3 grid;
    if (ensemble_v4(chw, {samples, mean, stdv}, B, &grid)) hipLaunchKernelGGL(ensemble_reduce_kernel<4>, grid, dim3(256), 0, s, samples, K, chw, mean, stdv);
    else hipLaunchKernelGGL(ensemble_reduce_kernel<1>, grid, dim3(256), 0, s, samples, K, chw, mean, stdv);
    return hipGetLastError();
}

// dst [n][chw] <- noisy[(v0 + j) / K]: the condition image of every virtual sample of one ensemble pass (the K members of an
// image share it).  grid (chunks of 256 * V elements, n); 8 bytes per element
template <int V>
__global__ __launch_bounds__(256)
void ensemble_broadcast_kernel(const float* __restrict__ noisy, float* __restrict__ dst, int v0, int K, unsigned long long chw) {
    const unsigned long long e = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (e >= chw) return;
    const size_t j = blockIdx.y, img = (size_t)((unsigned)v0 + blockIdx.y) / (unsigned)K;
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst + j * chw + e) = *reinterpret_cast<const f32x4*>(noisy + img * chw + e);
    else dst[j * chw + e] = noisy[img * chw + e];
}

hipError_t ensemble_broadcast_launch(const float* noisy, float* dst, int v0, int n, int K, unsigned long long chw, hipStream_t s) {
    if (v0 < 0 || n < 1 || n > 65535 || K < 1 || chw < 1 || chw >= (1ull << 32)) return hipErrorInvalidValue;
    dim3 grid;
    if (ensemble_v4(chw, {noisy, dst}, n, &grid)) hipLaunchKernelGGL(ensemble_broadcast_kernel<4>, grid, dim3(256), 0, s, noisy, dst, v0, K, chw);
    else hipLaunchKernelGGL(ensemble_broadcast_kernel<1>, grid, dim3(256), 0, s, noisy, dst, v0, K, chw);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ quantile maps over the members
// samples [B][K][chw] -> out [B][nq][chw]: per pixel the nq quantiles of its K members.  THE ARITHMETIC IS FIXED (include/midd.h:
// mi_ensemble_quantiles) and per pixel, so neither V, the alignment path nor the grid shows in the result: the members are sorted
// by their order keys (quantile_common.h), then per level, in double, every operation rounded on its own,
//   pos = q * (K - 1);  lo = floor(pos);  hi = min(lo + 1, K - 1);  g = pos - lo;  out = (float)(s_lo + g * (s_hi - s_lo))
// A thread owns V neighbouring pixels as ensemble_reduce_kernel does (V = 4: 16-byte loads and stores), loads its K members ONCE,
// keeps the KP >= K keys (K padded to a power of two with keys above +inf) in registers and sorts them with the unrolled network:
// every register index is a compile-time constant.  lo and hi are the same for every pixel (they depend on q and K alone), but
// they are run-time values: s_lo and s_hi are picked by a chain of selects, not by indexing the array, so nothing goes to scratch
// (tests/test_quantiles_cpu.py holds every instantiation to a private segment of 0 bytes).  The levels are kernel arguments.
// A pixel with a NaN member, and a NaN that the interpolation itself makes of infinite members, is the canonical quiet NaN.
template <int KP, int V>
__global__ __launch_bounds__(256)
void ensemble_quantiles_kernel(const float* __restrict__ samples, int K, unsigned long long chw, QuantileLevels ql, float* __restrict__ out) {
    const unsigned long long e = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (e >= chw) return;                                   // (V == 4: chw % 4 == 0, so e + 3 < chw)
    const size_t b = blockIdx.y;
    const float* src = samples + b * (size_t)K * chw + e;
    uint32_t key[V][KP];
    bool has_nan[V];
#pragma unroll
    for (int j = 0; j < V; ++j) has_nan[j] = false;
#pragma unroll
    for (int m = 0; m < KP; ++m) {
        if (m < K) {
            uint32_t x[V];
            if constexpr (V == 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)m * chw);
                x[0] = __float_as_uint(v.x); x[1] = __float_as_uint(v.y); x[2] = __float_as_uint(v.z); x[3] = __float_as_uint(v.w);
            } else {
                x[0] = __float_as_uint(src[(size_t)m * chw]);
            }
#pragma unroll
            for (int j = 0; j < V; ++j) { key[j][m] = order_key(x[j]); has_nan[j] = has_nan[j] || is_nan_bits(x[j]); }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) key[j][m] = ORDER_KEY_PAD;
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) sort_keys<KP>(key[j]);
    float* dst = out + b * (size_t)ql.nq * chw + e;
    for (int i = 0; i < ql.nq; ++i) {
        const QuantilePos p = quantile_pos(ql.q[i], K);
        float r[V];
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = quantile_of_sorted<KP>(key[j], p, K, has_nan[j]);
        if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst + (size_t)i * chw) = (f32x4){r[0], r[1], r[2], r[3]};
        else dst[(size_t)i * chw] = r[0];
    }
}

template <int KP>
static void ensemble_quantiles_dispatch(const float* samples, int B, int K, unsigned long long chw, const QuantileLevels& ql, float* out, hipStream_t s) {
    dim3 grid;
    if (ensemble_v4(chw, {samples, out}, B, &grid)) hipLaunchKernelGGL((ensemble_quantiles_kernel<KP, 4>), grid, dim3(256), 0, s, samples, K, chw, ql, out);
    else hipLaunchKernelGGL((ensemble_quantiles_kernel<KP, 1>), grid, dim3(256), 0, s, samples, K, chw, ql, out);
}

hipError_t ensemble_quantiles_launch(const float* samples, int B, int K, unsigned long long chw, const QuantileLevels& ql, float* out, hipStream_t s) {
    if (B < 1 || B > 65535 || K < 1 || K > QUANTILE_MAX_MEMBERS || chw < 1 || chw >= (1ull << 32) || !samples || !out || !quantile_levels_ok(ql))
        return hipErrorInvalidValue;
    if (K <= 2) ensemble_quantiles_dispatch<2>(samples, B, K, chw, ql, out, s);
    else if (K <= 4) ensemble_quantiles_dispatch<4>(samples, B, K, chw, ql, out, s);
    else if (K <= 8) ensemble_quantiles_dispatch<8>(samples, B, K, chw, ql, out, s);
    else if (K <= 16) ensemble_quantiles_dispatch<16>(samples, B, K, chw, ql, out, s);
    else if (K <= 32) ensemble_quantiles_dispatch<32>(samples, B, K, chw, ql, out, s);
    else ensemble_quantiles_dispatch<64>(samples, B, K, chw, ql, out, s);
    return hipGetLastError();
}

}  // namespace midd
