// Geometry of tiled denoising (include/midd.h: mi_tile_geometry, mi_denoise_tiled): ONE set of functions for the host checks,
// the extract / blend kernels (tiles.hip) and the seeded update (out_conv.hip); tests/tiled_reference.py restates it in numpy.
// Per axis: an image length L is covered by n tiles of length T whose neighbours overlap by at least O (0 <= O <= T/2, T <= L):
//   n = 1 if L == T, else max(2, ceil((L - O) / (T - O)))
//   origin of tile i:  o_i = floor(i * (L - T) / (n - 1))   (o_0 = 0, o_{n-1} = L - T; n == 1: o_0 = 0)
//   window inside a tile, position r in [0, T):  w(r) = min(r + 1, T - r, O + 1)   -- an integer ramp of O + 1 steps at either end
// A tile's blend weight is wy * wx.  Tiles of an image are numbered k = ky * nx + kx.
#pragma once
#include <hip/hip_runtime.h>

namespace midd {

__host__ __device__ __forceinline__ int tile_count(int L, int T, int O) {
    if (L == T) return 1;
    const int n = (L - O + (T - O) - 1) / (T - O);
    return n < 2 ? 2 : n;
}

__host__ __device__ __forceinline__ int tile_origin(int i, int L, int T, int n) {
    return n <= 1 ? 0 : (int)((long long)i * (L - T) / (n - 1));
}

__host__ __device__ __forceinline__ int tile_window(int r, int T, int O) {
    const int a = r + 1, b = T - r, c = O + 1;
    const int m = a < b ? a : b;
    return m < c ? m : c;
}

// the tiles of one axis that cover position p, as the index range [*first, *last] (ascending origins; never empty for 0 <= p < L)
__host__ __device__ __forceinline__ void tile_cover(int p, int L, int T, int n, int* first, int* last) {
    int hi = (n <= 1) ? 0 : (int)((long long)p * (n - 1) / (L - T));       // near the last tile whose origin is <= p
    if (hi > n - 1) hi = n - 1;
    while (hi + 1 < n && tile_origin(hi + 1, L, T, n) <= p) ++hi;
    while (hi > 0 && tile_origin(hi, L, T, n) > p) --hi;
    int lo = hi;
    while (lo > 0 && tile_origin(lo - 1, L, T, n) + T > p) --lo;
    *first = lo; *last = hi;
}

}  // namespace midd
