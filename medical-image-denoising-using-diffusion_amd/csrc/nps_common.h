// What the Welch spectra share (nps.hip: THE NOISE POWER SPECTRUM; cross_spectrum.hip: THE CROSS SPECTRUM).  The stages of an ROI
// kernel, each described once here; what is also code here is named:
//   walk      a workgroup owns ONE chunk of NPS_CHUNK = 16 consecutive ROIs of one group and walks them in order (nps_walk)
//   load      a lane's row quads (nps_load_quads): 16-byte loads when W is a multiple of 4 and the ROI's first element is 16-byte
//             aligned, element loads otherwise, the same values; a non-finite value marks the ROI skipped
//   detrend   the field goes to the plane in natural order; one lane per row adds it (s0 = sum f, s1 = sum xc f, x from 0), one lane
//             adds the rows (y from 0) and forms m, ax, ay; every element is detrended in double, rounded once, multiplied by w[y] and
//             then by w[x], and written at [bitrev(y)][bitrev(x)]
//   passes    log2 R radix-2 decimation-in-time stages in place (nps_butterfly), over all R rows -- consecutive lanes take consecutive
//             ROWS at one butterfly index: odd pitch, so the 32 lanes of a half wave are on 32 different bank pairs, and the twiddle
//             is one broadcast read -- and then over the columns, consecutive lanes on consecutive columns
//   sums      the lane's double accumulators take the chunk's ROIs in order; chunk sums and used counts go to the workspace; one lane
//             per entry adds the group's chunk sums from 0 in chunk order (nps_chunk_sum), entry and mirror (nps_store_mirrored)
//   bins      nps_radial_kernel<R>: one wave per (group, bin) over the group's plane in LDS: the rows in order, per row one ballot
//             over the columns and the bin's entries added in ascending column order, i.e. row-major
// The row sums, the coefficients, the element's detrend and the two stage loops are written out in each ROI kernel: as shared inline
// functions each of them changed a kernel's code (profiles/nps_isa.txt, profiles/cross_spectrum_isa.txt).  LDS of an ROI kernel: ONE
// complex plane of interleaved (re, im) words, R rows with pitch R + 1 words, the tables and the row sums.  No atomics.  Contraction
// is off: a complex multiply is four v_mul_f32 and two v_add/v_sub_f32.
#pragma once
#include "midd_internal.h"
#include <type_traits>
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

// The ROI walk of a workgroup: the chunk's ROIs [r0, r1) of the group's n_rois, and per ROI the member m and the place rem among
// the member's ny * nx positions (< 2^31: the entry's rule).  for (r = w.r0; r < w.r1; ++r, ++w.rem) { nps_walk_roi(w, ...); ... }
struct NpsWalk { unsigned long long r0, r1; unsigned per_member; size_t m; unsigned rem; };
__device__ __forceinline__ NpsWalk nps_walk(unsigned chunk, unsigned long long n_rois, int ny, int nx) {
    const unsigned long long r0 = (unsigned long long)chunk * NPS_CHUNK;
    const unsigned per_member = (unsigned)ny * (unsigned)nx;
    return {r0, r0 + NPS_CHUNK < n_rois ? r0 + NPS_CHUNK : n_rois, per_member, (size_t)(r0 / per_member), (unsigned)(r0 % per_member)};
}

// the ROI's member (w.m) and origin (oy, ox)
__device__ __forceinline__ void nps_walk_roi(NpsWalk& w, int nx, int S, size_t& oy, size_t& ox) {
    if (w.rem == w.per_member) { w.rem = 0; ++w.m; }
    oy = (size_t)(w.rem / (unsigned)nx) * S, ox = (size_t)(w.rem % (unsigned)nx) * S;
}

// the denominator of the plane's slopes, D = R * (R (R^2 - 1) / 12): exact integers
template <int R> constexpr double NPS_SLOPE_DEN = (double)R * ((double)R * ((double)R * R - 1.0) / 12.0);

// an entry's chunk sums p[c * PITCH], one by one from 0 in chunk order; BATCH independent loads are in flight per step of the
// dependent chain of adds
template <int BATCH, size_t PITCH>
__device__ __forceinline__ double nps_chunk_sum(const double* p, unsigned chunks) {
    double s = 0.0;
    unsigned c = 0;
    for (; c + BATCH <= chunks; c += BATCH) {
        double v[BATCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) v[j] = p[(size_t)(c + j) * PITCH];
#pragma unroll
        for (int j = 0; j < BATCH; ++j) s = add_rn64(s, v[j]);
    }
    for (; c < chunks; ++c) s = add_rn64(s, p[(size_t)c * PITCH]);
    return s;
}

// entry idx = (v, u) of the half plane in plane [q][g] of planes [..][groups][R][R] and, for 0 < u < R/2, its mirror ((R - v) % R, R - u)
template <int R>
__device__ __forceinline__ void nps_store_mirrored(double* planes, size_t q, size_t groups, size_t g, int idx, double val, double mirror) {
    const int v = idx / NpsGeom<R>::NC, u = idx % NpsGeom<R>::NC;
    double* out = planes + (q * groups + g) * (size_t)(R * R);
    out[v * R + u] = val;
    if (u > 0 && u < R / 2) out[((R - v) % R) * R + (R - u)] = mirror;
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

// ---------------------------------------------------------------------------------------------------------------- host
// the ROI positions of a member, the ROIs of a group and its chunks of NPS_CHUNK
struct NpsCounts { int ny, nx; unsigned long long n_rois, chunks; };
inline NpsCounts nps_counts(int K, int H, int W, int R, int S) {
    const int ny = (H - R) / S + 1, nx = (W - R) / S + 1;
    const unsigned long long n_rois = (unsigned long long)K * (unsigned long long)ny * (unsigned long long)nx;
    return {ny, nx, n_rois, (n_rois + NPS_CHUNK - 1) / NPS_CHUNK};
}

// f(std::integral_constant<int, R>{}) for the ROI size R in {32, 64, 128} (the entry's rule): the launches of a call, instantiated
// for the three sizes
template <class F>
hipError_t nps_for_roi_size(int R, F f) {
    if (R == 32) return f(std::integral_constant<int, 32>{});
    if (R == 64) return f(std::integral_constant<int, 64>{});
    return f(std::integral_constant<int, 128>{});
}

}  // namespace midd
