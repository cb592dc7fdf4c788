// What the Welch spectra share (nps.hip: THE NOISE POWER SPECTRUM; cross_spectrum.hip: THE CROSS SPECTRUM): the geometry of an ROI's
// half plane, the finite test, the row-quad loads, the single-product butterfly and the radial bins.
#pragma once
#include "midd_internal.h"
#include "pointwise_common.h"

#pragma clang fp contract(off)

namespace midd {

constexpr int NPS_THREADS = 256;
static_assert(NPS_CHUNK == 16, "THE NOISE POWER SPECTRUM: chunks of 16 consecutive ROIs");
constexpr unsigned long long NPS_QNAN = 0x7FF8000000000000ull;

__device__ __forceinline__ bool nps_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

template <int R> struct NpsGeom {
    static constexpr int LOG = R == 32 ? 5 : R == 64 ? 6 : 7;
    static constexpr int NC = R / 2 + 1;                 // columns kept by the column pass
    static constexpr int P = R + 1;                      // LDS pitch in floats
    static constexpr int HALF = R * NC;                  // entries of the half plane
    static constexpr int NACC = (HALF + NPS_THREADS - 1) / NPS_THREADS;
};

__device__ __forceinline__ bool nps_aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// a lane's row quads of one ROI plane: 16-byte loads (V = 4) or four element loads each (V = 1), all issued before any is used.  The
// choice is made once per ROI and is uniform over the workgroup: a choice per quad is a divergent branch around every load, which
// waits for each load on its own
template <int R, int NQ, int V, int T = NPS_THREADS>
__device__ __forceinline__ void nps_load_quads(const float* __restrict__ p, size_t W, int tid, f32x4 (&v)[NQ]) {
#pragma unroll
    for (int e = 0; e < NQ; ++e) {
        const int q = tid + T * e, y = q / (R / 4), x4 = (q % (R / 4)) * 4;
        const float* src = p + (size_t)y * W + x4;
        if constexpr (V == 4) v[e] = *reinterpret_cast<const f32x4*>(src);
        else v[e] = (f32x4){src[0], src[1], src[2], src[3]};
    }
}

// One fp32 product as one v_mul_f32.  Left to the compiler the four products of a butterfly pair up as v_pk_mul_f32 with an op_sel
// bit (the twiddle component broadcast from the high half of its register pair), the form tools/isa_hazard_audit.py bans
__device__ __forceinline__ float nps_mul(float a, float b) {
    float r;
    asm("v_mul_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// one radix-2 decimation-in-time butterfly on (ia, ib) with twiddle w: t = w * z[ib] as four products and two sums
__device__ __forceinline__ void nps_butterfly(float2* z, int ia, int ib, float2 w) {
    const float2 x = z[ib], u = z[ia];
    const float tr = nps_mul(w.x, x.x) - nps_mul(w.y, x.y);
    const float ti = nps_mul(w.x, x.y) + nps_mul(w.y, x.x);
    z[ia] = make_float2(u.x + tr, u.y + ti);
    z[ib] = make_float2(u.x - tr, u.y - ti);
}

// grid (ceil((R/2 + 1) / 4), groups), one wave per bin.  The workgroup first copies the group's plane to LDS (R^2 doubles: 8, 32 and
// 128 KiB): a bin's entries are added one after the other, and from global memory every one of them was a dependent round trip
template <int R>
__global__ __launch_bounds__(NPS_THREADS)
void nps_radial_kernel(const double* __restrict__ nps, const long long* __restrict__ rois_used, int exclude_axes,
                       double* __restrict__ radial, long long* __restrict__ radial_count) {
    __shared__ double plane[R * R];
    const size_t g = blockIdx.y;
    const double* src = nps + g * (size_t)(R * R);
#pragma unroll 4
    for (int i = threadIdx.x; i < R * R; i += NPS_THREADS) plane[i] = src[i];
    __syncthreads();
    const int r = blockIdx.x * (NPS_THREADS / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r > R / 2) return;
    const int lo = (2 * r - 1) * (2 * r - 1), hi = (2 * r + 1) * (2 * r + 1);
    double s = 0.0;
    long long cnt = 0;
#pragma unroll 2
    for (int v = 0; v < R; ++v) {
        const int fv = v < R / 2 ? v : v - R;
        for (int ub = 0; ub < R; ub += 64) {
            const int u = ub + lane;
            const int fu = u < R / 2 ? u : u - R;
            const int d4 = 4 * (fu * fu + fv * fv);
            bool in = u < R && (r == 0 || lo <= d4) && d4 < hi;
            if (exclude_axes && (fu == 0 || fv == 0)) in = false;
            const double val = plane[v * R + (u < R ? u : 0)];
            unsigned long long mask = __ballot(in);
            while (mask) {                                  // ascending columns: row-major
                const int bit = __ffsll((long long)mask) - 1;
                s = add_rn64(s, __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(val), bit), __builtin_amdgcn_readlane(__double2loint(val), bit)));
                ++cnt;
                mask &= mask - 1;
            }
        }
    }
    if (lane == 0) {
        const bool none = cnt == 0 || rois_used[g] == 0;
        radial[g * (R / 2 + 1) + r] = none ? __longlong_as_double((long long)NPS_QNAN) : __ddiv_rn(s, (double)cnt);
        if (g == 0) radial_count[r] = cnt;
    }
}

}  // namespace midd
