// The responses of image planes to channel templates at given locations (include/midd.h: THE CHANNEL RESPONSES;
// tests/observer_reference.py restates it in numpy): out[n][l][c] = sum over the R x R region of interest (ROI) l of plane n of
// channels[c][p] * x[n][y0 + y][x0 + x], p = y R + x, in double precision and in ONE order.  It is the hot path of the channelized
// Hotelling observer (observer.py): everything after it works on [rows, C] doubles on the host.
//   channel_responses_kernel    A wave owns CR_PLANES ROIs: the same location in consecutive planes.  Lane j walks the elements
//                               p = j, j + 64, .. of the ROI, so a wave's loads of a plane are runs of consecutive floats (a whole
//                               row of the ROI, or several), and its loads of a channel are 512 consecutive bytes.  A channel value
//                               a lane has loaded serves all of the wave's planes, and the CR_WAVES waves of a workgroup walk the
//                               same location in step, so the channel tile comes from L2 once per workgroup and from the vector
//                               cache after that.  The channels go in blocks of at most CR_BLOCK accumulators per plane (1, 2, 4 or
//                               8, the smallest that holds what is left); a further block walks the ROI again, from the cache.
//                               The 64 lane sums are folded by the tree v[j] += v[j + off], off = 32 .. 1, across the lanes (no
//                               LDS) and lane 0 stores: no atomics, and nothing of the launch geometry in the order.
// The planes are read element by element, whatever the alignment of x, x0 or W: there is one load path, so the alignment cannot show.
// No matrix instruction: the order in which a double MFMA adds its products is not specified, so it could not be held to the
// restatement (as in ensemble_modes.hip).  Contraction is off for the whole unit; sums and products go through the *_rn64 helpers.
// The ROI origins are HOST integers, judged by the ABI before any GPU work, and travel as kernel arguments, CR_CENTRES a launch: the
// call needs no workspace, and more locations than that are further launches of the same arithmetic.
#include "midd_internal.h"
#include "pointwise_common.h"

#pragma clang fp contract(off)

namespace midd {

constexpr int CR_LANES = 64;
constexpr int CR_WAVES = 4;                                           // waves of a workgroup: the same location, consecutive plane groups
constexpr int CR_PLANES = 2;                                          // planes (ROIs) of a wave
constexpr int CR_BLOCK = 8;                                           // accumulators per plane and lane
constexpr int CR_CENTRES = 512;                                       // locations of a launch: 2 KiB of kernel arguments
struct ChannelOrigins { uint32_t yx[CR_CENTRES]; };                   // y0 << 16 | x0 (H, W <= 32768)

__device__ __forceinline__ bool cr_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }

// one block of CB channels, c0 .. c0 + CB - 1 (a channel past C is channel C - 1 again: always there, never stored), over the
// wave's CR_PLANES ROIs; roi[q] points at the ROI's first element, pitch W; row is (n0, l) as n0 L + l.  Lane 0 stores the block's
// responses, and with the first block the ROI's invalid flag (every block sees every pixel)
template <int CB>
__device__ __forceinline__ void cr_block(const float* const (&roi)[CR_PLANES], const bool (&present)[CR_PLANES], int W, int R,
                                         const double* __restrict__ channels, int C, int c0, int lane, size_t row,
                                         double* __restrict__ out, uint32_t* __restrict__ invalid, int L) {
    const int RR = R * R;
    const double* u[CB];
#pragma unroll
    for (int t = 0; t < CB; ++t) u[t] = channels + (size_t)(c0 + t < C ? c0 + t : C - 1) * RR;
    double acc[CR_PLANES][CB];
    bool finite[CR_PLANES];
#pragma unroll
    for (int q = 0; q < CR_PLANES; ++q) {
        finite[q] = true;
#pragma unroll
        for (int t = 0; t < CB; ++t) acc[q][t] = 0.0;
    }
    // lane j is at element p = j + 64 k of the ROI: (y, x) moves by (64 / R, 64 % R) with a carry
    const int dy = CR_LANES / R, dx = CR_LANES - dy * R;
    int y = lane / R, x = lane - y * R;
    for (int p = lane; p < RR; p += CR_LANES) {
        const unsigned o = (unsigned)y * (unsigned)W + (unsigned)x;
        float g[CR_PLANES];
        double w[CB];
#pragma unroll
        for (int q = 0; q < CR_PLANES; ++q) g[q] = roi[q][o];
#pragma unroll
        for (int t = 0; t < CB; ++t) w[t] = u[t][p];
#pragma unroll
        for (int q = 0; q < CR_PLANES; ++q) {
            finite[q] = finite[q] && cr_finite(g[q]);
            const double gd = (double)g[q];
#pragma unroll
            for (int t = 0; t < CB; ++t) acc[q][t] = add_rn64(acc[q][t], mul_rn64(w[t], gd));
        }
        x += dx;
        y += dy;
        if (x >= R) { x -= R; ++y; }
    }
#pragma unroll
    for (int off = CR_LANES / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int q = 0; q < CR_PLANES; ++q) {
#pragma unroll
            for (int t = 0; t < CB; ++t) acc[q][t] = add_rn64(acc[q][t], __shfl_down(acc[q][t], (unsigned)off, CR_LANES));
        }
    }
    const double qnan = __longlong_as_double(0x7FF8000000000000ll);
#pragma unroll
    for (int q = 0; q < CR_PLANES; ++q) {
        const bool bad = __any(finite[q] ? 0 : 1) != 0;
        if (lane == 0 && present[q]) {
            const size_t r = row + (size_t)q * L;                     // (n, l) as n L + l
            if (c0 == 0) invalid[r] = bad ? 1u : 0u;
#pragma unroll
            for (int t = 0; t < CB; ++t)
                if (c0 + t < C) out[r * C + c0 + t] = bad ? qnan : acc[q][t];
        }
    }
}

// grid (locations of the launch, plane groups of CR_WAVES * CR_PLANES planes); l0: the launch's first location
__global__ __launch_bounds__(CR_LANES * CR_WAVES)
void channel_responses_kernel(const float* __restrict__ x, int N, int H, int W, ChannelOrigins org, int l0, int L, int R,
                              const double* __restrict__ channels, int C, double* __restrict__ out, uint32_t* __restrict__ invalid) {
    const int lane = threadIdx.x & (CR_LANES - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / CR_LANES);
    const int n0 = (blockIdx.y * CR_WAVES + wave) * CR_PLANES;
    if (n0 >= N) return;
    const uint32_t yx = org.yx[blockIdx.x];
    const size_t first = (size_t)(yx >> 16) * W + (yx & 0xFFFFu);
    const float* roi[CR_PLANES];
    bool present[CR_PLANES];
#pragma unroll
    for (int q = 0; q < CR_PLANES; ++q) {                             // a plane past N is plane N - 1 again, never stored
        present[q] = n0 + q < N;
        roi[q] = x + (size_t)(present[q] ? n0 + q : N - 1) * H * W + first;
    }
    const size_t row = (size_t)n0 * L + (size_t)(l0 + (int)blockIdx.x);
    for (int c0 = 0; c0 < C; c0 += CR_BLOCK) {
        const int rest = C - c0;
        if (rest > 4) cr_block<8>(roi, present, W, R, channels, C, c0, lane, row, out, invalid, L);
        else if (rest > 2) cr_block<4>(roi, present, W, R, channels, C, c0, lane, row, out, invalid, L);
        else if (rest > 1) cr_block<2>(roi, present, W, R, channels, C, c0, lane, row, out, invalid, L);
        else cr_block<1>(roi, present, W, R, channels, C, c0, lane, row, out, invalid, L);
    }
}

// centres: HOST int32 [L][2] as (cy, cx), every ROI inside the image (the ABI has judged that)
hipError_t channel_responses_launch(const float* x, int N, int H, int W, const int32_t* centres, int L, int R, const double* channels, int C,
                                    double* out, uint32_t* invalid, hipStream_t s) {
    if (N < 1 || N > CR_MAX_PLANES || H < 1 || H > CR_MAX_SIDE || W < 1 || W > CR_MAX_SIDE || R < CR_MIN_ROI || R > CR_MAX_ROI || L < 1 ||
        L > CR_MAX_LOCATIONS || C < 1 || C > CR_MAX_CHANNELS || !x || !centres || !channels || !out || !invalid)
        return hipErrorInvalidValue;
    const unsigned groups = (unsigned)((N + CR_WAVES * CR_PLANES - 1) / (CR_WAVES * CR_PLANES));
    for (int l0 = 0; l0 < L; l0 += CR_CENTRES) {
        const int n = L - l0 < CR_CENTRES ? L - l0 : CR_CENTRES;
        ChannelOrigins org{};
        for (int i = 0; i < n; ++i) {
            const int y0 = centres[2 * (l0 + i)] - R / 2, x0 = centres[2 * (l0 + i) + 1] - R / 2;
            if (y0 < 0 || x0 < 0 || y0 + R > H || x0 + R > W) return hipErrorInvalidValue;
            org.yx[i] = (uint32_t)y0 << 16 | (uint32_t)x0;
        }
        hipLaunchKernelGGL(channel_responses_kernel, dim3((unsigned)n, groups), dim3(CR_LANES * CR_WAVES), 0, s, x, N, H, W, org, l0, L, R,
                           channels, C, out, invalid);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace midd
