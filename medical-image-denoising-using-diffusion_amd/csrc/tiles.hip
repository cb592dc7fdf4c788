// HBM-bound streams between a larger image and its overlapping network-sized tiles.
//
//   tile_extract_kernel / tile_blend_kernel : overlapping network-sized tiles of a larger image, and their blend (mi_denoise_tiled)
//   tile_blend_reduce_kernel : blend of every member's tiles and mean / std over the blended members (mi_denoise_tiled_ensemble)
//   tile_blend_quantiles_kernel : per-pixel quantiles over the members, blended from tiles
#include "midd_internal.h"
#include "tile_geometry.h"
#include "quantile_common.h"

namespace midd {

// ------------------------------------------------------------------------------ tiled denoising: extract and blend
// Both are HBM-bound streams over the image (tile_geometry.h holds the geometry; origins come from its formula, no table in
// memory).  Extract: grid (chunks of 256 threads over C * th * tw / V, n virtual samples); the tile is uniform in the
// workgroup, so its origin is scalar arithmetic.  V = 4: a thread moves four neighbouring pixels of one tile row and stores them
// as 16 bytes (tw % 4 == 0, dst 16-byte aligned); it LOADS them as 16 bytes when the source address allows (row pitch W % 4 == 0,
// noisy 16-byte aligned -- `vload` -- and this tile's x0 % 4 == 0), else as four dwords.  V = 1: one dword per thread, any shape.
template <int V>
__global__ __launch_bounds__(256)
void tile_extract_kernel(const float* __restrict__ noisy, float* __restrict__ dst, TileGeom g, int v0, int vload) {
    const unsigned e = (blockIdx.x * 256u + threadIdx.x) * V;                 // element inside the tile block [C][th][tw]
    const unsigned tile_elems = (unsigned)g.C * g.th * g.tw;
    if (e >= tile_elems) return;
    const unsigned v = (unsigned)v0 + blockIdx.y, K = (unsigned)(g.ny * g.nx);
    const unsigned img = v / K, k = v - img * K;
    const int ky = (int)k / g.nx, kx = (int)k - ky * g.nx;
    const int y0 = tile_origin(ky, g.H, g.th, g.ny), x0 = tile_origin(kx, g.W, g.tw, g.nx);
    const unsigned x = e % (unsigned)g.tw, cy = e / (unsigned)g.tw;
    const unsigned y = cy % (unsigned)g.th, c = cy / (unsigned)g.th;
    const float* src = noisy + (((size_t)img * g.C + c) * g.H + (y0 + y)) * (size_t)g.W + x0 + x;
    float* out = dst + (size_t)blockIdx.y * tile_elems + e;
    if constexpr (V == 4) {
        f32x4 r;
        if (vload && (x0 & 3) == 0) r = *reinterpret_cast<const f32x4*>(src);
        else r = (f32x4){src[0], src[1], src[2], src[3]};
        *reinterpret_cast<f32x4*>(out) = r;
    } else {
        *out = *src;
    }
}

hipError_t tile_extract_launch(const float* noisy, float* dst, const TileGeom& g, int v0, int n, hipStream_t s) {
    if (v0 < 0 || n < 1 || n > 65535 || g.C < 1 || g.ny < 1 || g.nx < 1 || g.th < 1 || g.tw < 1 || g.th > g.H || g.tw > g.W ||
        (unsigned long long)g.C * g.th * g.tw >= (1ull << 31)) return hipErrorInvalidValue;
    const unsigned tile_elems = (unsigned)g.C * g.th * g.tw;
    if (g.tw % 4 == 0 && aligned16(dst))
        hipLaunchKernelGGL(tile_extract_kernel<4>, dim3((tile_elems / 4 + 255) / 256, n), dim3(256), 0, s, noisy, dst, g, v0,
                           (g.W % 4 == 0 && aligned16(noisy)) ? 1 : 0);
    else
        hipLaunchKernelGGL(tile_extract_kernel<1>, dim3((tile_elems + 255) / 256, n), dim3(256), 0, s, noisy, dst, g, v0, 0);
    return hipGetLastError();
}

// Blend, as a gather: a thread owns ONE output pixel, finds the tiles that cover it from the origin formula (tile_cover: at most
// three per axis for every geometry the host accepts, but the loop does not rely on it) and walks them in ascending (ky, kx).
// THE ARITHMETIC IS FIXED (include/midd.h: mi_tile_blend) and per pixel: in double, every operation rounded on its own,
//   num += (double)(wy * wx) * (double)v;   den += (double)(wy * wx);   out = (float)(num / den)
// with the integer windows of tile_geometry.h.  No atomics, nothing depends on the launch geometry; a pixel under one tile gets
// that tile's value back exactly (w * v is exact in double, and so is the quotient).  Neighbouring threads read neighbouring
// floats of the same tile row: every wave instruction is a contiguous run (broken once where a tile boundary crosses the wave).
// grid (chunks of 256 pixels of a [C][H][W] block, images -- folded over grid.y when B > 65535)
__global__ __launch_bounds__(256)
void tile_blend_kernel(const float* __restrict__ tiles, float* __restrict__ out, int B, TileGeom g) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (e >= chw) return;
    const int x = (int)(e % (unsigned)g.W);
    const unsigned long long cy = e / (unsigned)g.W;
    const int y = (int)(cy % (unsigned)g.H), c = (int)(cy / (unsigned)g.H);
    int ky0, ky1, kx0, kx1;
    tile_cover(y, g.H, g.th, g.ny, &ky0, &ky1);
    tile_cover(x, g.W, g.tw, g.nx, &kx0, &kx1);
    const size_t tile_plane = (size_t)g.th * g.tw, K = (size_t)g.ny * g.nx;
    for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) {
        double num = 0.0, den = 0.0;
        for (int ky = ky0; ky <= ky1; ++ky) {
            const int ry = y - tile_origin(ky, g.H, g.th, g.ny);
            const int wy = tile_window(ry, g.th, g.oy);
            for (int kx = kx0; kx <= kx1; ++kx) {
                const int rx = x - tile_origin(kx, g.W, g.tw, g.nx);
                const double w = (double)(wy * tile_window(rx, g.tw, g.ox));
                const float v = tiles[((b * K + (size_t)ky * g.nx + kx) * g.C + c) * tile_plane + (size_t)ry * g.tw + rx];
                num = add_rn64(num, mul_rn64(w, (double)v));
                den = add_rn64(den, w);
            }
        }
        out[b * chw + e] = __double2float_rn(__ddiv_rn(num, den));
    }
}

// What every blend launch refuses in (B, g): a tile outside the image, chw >= 2^32, a window product wy * wx that does not fit an
// int (oy + 1, ox + 1 <= 46340).  grid (chunks of 256 elements of a [C][H][W] block, images folded over grid.y when B > 65535)
static bool tile_blend_geom_ok(int B, const TileGeom& g, dim3* grid) {
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (B < 1 || g.C < 1 || g.ny < 1 || g.nx < 1 || g.th < 1 || g.tw < 1 || g.th > g.H || g.tw > g.W || chw >= (1ull << 32) ||
        g.oy < 0 || g.ox < 0 || (long long)g.oy + 1 > 46340 || (long long)g.ox + 1 > 46340) return false;
    *grid = dim3((unsigned)((chw + 255) / 256), B < 65535 ? B : 65535);
    return true;
}

// The tile blocks of M members, B * ny * nx * M, are indexed by an int (after tile_blend_geom_ok)
static bool tile_blocks_ok(int B, int M, const TileGeom& g) {
    const long long BK = (long long)B * ((long long)g.ny * g.nx);            // (ny * nx <= H * W < 2^32: no overflow in either product)
    return BK <= 2147483647ll && BK * M <= 2147483647ll;
}

hipError_t tile_blend_launch(const float* tiles, float* out, int B, const TileGeom& g, hipStream_t s) {
    dim3 grid;
    if (!tile_blend_geom_ok(B, g, &grid)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tile_blend_kernel, grid, dim3(256), 0, s, tiles, out, B, g);
    return hipGetLastError();
}

// Blend and reduce in one pass over the image (mi_denoise_tiled_ensemble): tiles [M][B][ny*nx][C][th][tw], the tile outputs of M
// members in run order, -> mean / unbiased std [B][C][H][W] over the members' BLENDED images and, if asked for, those images
// themselves, samples [B][M][C][H][W].  A thread owns ONE output element of one image, as in tile_blend_kernel, whose addressing
// this keeps (member m, image b is the tile block m * B + b).  THE ARITHMETIC IS FIXED (include/midd.h: mi_tile_blend_reduce):
// the composition of the two kernels above, bit for bit --
//   v_m = (float)(num / den) of member m, formed as tile_blend_kernel forms it;  then over v_0 .. v_{M-1}, in index order, the
//   sums of ensemble_reduce_kernel: mean64 = (sum (double)v_m) / M,  q = sum d * d with d = (double)v_m - mean64
// M is a run-time value, so the v_m are not kept: the second walk (std only) blends them again from the tiles -- the same loads
// and the same operations, hence the same bits, whether or not samples is written; nothing is read back from samples.  The
// blended members never exist in memory unless the caller wants them: per pixel (1 or 2) * M * cover tile reads and 1-2 writes,
// against M * cover reads + M writes + 2 * M reads + 2 writes of blend-then-reduce.  No atomics, nothing depends on the grid.
// grid (chunks of 256 elements of a [C][H][W] block, images -- folded over grid.y when B > 65535)
__global__ __launch_bounds__(256)
void tile_blend_reduce_kernel(const float* __restrict__ tiles, float* __restrict__ mean, float* __restrict__ stdv,
                              float* __restrict__ samples, int B, int M, TileGeom g) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (e >= chw) return;
    const int x = (int)(e % (unsigned)g.W);
    const unsigned long long cy = e / (unsigned)g.W;
    const int y = (int)(cy % (unsigned)g.H), c = (int)(cy / (unsigned)g.H);
    int ky0, ky1, kx0, kx1;
    tile_cover(y, g.H, g.th, g.ny, &ky0, &ky1);
    tile_cover(x, g.W, g.tw, g.nx, &kx0, &kx1);
    const size_t tile_plane = (size_t)g.th * g.tw, K = (size_t)g.ny * g.nx;
    for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) {
        auto blended = [&](int m) -> float {                       // tile_blend_kernel's pixel, of tile block m * B + b
            const size_t mb = (size_t)m * B + b;
            double num = 0.0, den = 0.0;
            for (int ky = ky0; ky <= ky1; ++ky) {
                const int ry = y - tile_origin(ky, g.H, g.th, g.ny);
                const int wy = tile_window(ry, g.th, g.oy);
                for (int kx = kx0; kx <= kx1; ++kx) {
                    const int rx = x - tile_origin(kx, g.W, g.tw, g.nx);
                    const double w = (double)(wy * tile_window(rx, g.tw, g.ox));
                    const float v = tiles[((mb * K + (size_t)ky * g.nx + kx) * g.C + c) * tile_plane + (size_t)ry * g.tw + rx];
                    num = add_rn64(num, mul_rn64(w, (double)v));
                    den = add_rn64(den, w);
                }
            }
            return __double2float_rn(__ddiv_rn(num, den));
        };
        double sum = 0.0;
        for (int m = 0; m < M; ++m) {
            const float v = blended(m);
            if (samples) samples[(b * (size_t)M + m) * chw + e] = v;
            sum = add_rn64(sum, (double)v);
        }
        const double m64 = __ddiv_rn(sum, (double)M);
        if (mean) mean[b * chw + e] = __double2float_rn(m64);
        if (stdv) {
            double q = 0.0;
            for (int m = 0; m < M; ++m) {
                const double d = sub_rn64((double)blended(m), m64);
                q = add_rn64(q, mul_rn64(d, d));
            }
            stdv[b * chw + e] = __double2float_rn(__dsqrt_rn(__ddiv_rn(q, (double)(M - 1))));
        }
    }
}

hipError_t tile_blend_reduce_launch(const float* tiles, int B, int M, const TileGeom& g, float* mean, float* stdv, float* samples, hipStream_t s) {
    dim3 grid;
    if (!tile_blend_geom_ok(B, g, &grid) || M < 1 || (!mean && !stdv && !samples) || (stdv && M < 2)) return hipErrorInvalidValue;
    if (!tile_blocks_ok(B, M, g)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tile_blend_reduce_kernel, grid, dim3(256), 0, s, tiles, mean, stdv, samples, B, M, g);
    return hipGetLastError();
}

// Blend and quantiles in one pass over the image (mi_tile_blend_quantiles): tiles [M][B][ny*nx][C][th][tw] -> out [B][nq][C][H][W],
// the quantiles over the members' BLENDED images, which never exist in memory.  A thread owns ONE output element of one image
// with the addressing of tile_blend_reduce_kernel.  THE ARITHMETIC IS FIXED: v_m = (float)(num_m / den) exactly as
// tile_blend_kernel forms it -- the covering tiles in ascending (ky, kx), num_m += (double)(wy * wx) * (double)v -- for every member
// once, then the sort and the interpolation of ensemble_quantiles_kernel over v_0 .. v_{M-1}: the output equals mi_tile_blend of
// every member followed by mi_ensemble_quantiles, bit for bit.  The tile walk is the outer loop and the members the unrolled inner
// one: the windows are formed once per tile, a tile's M loads are in flight together, and every member still sees its own
// additions in the same order (den is the same sum for every member).  KP doubles and KP keys per thread, all at constant indices.
// grid (chunks of 256 elements of a [C][H][W] block, images -- folded over grid.y when B > 65535)
template <int KP>
__global__ __launch_bounds__(256)
void tile_blend_quantiles_kernel(const float* __restrict__ tiles, float* __restrict__ out, int B, int M, TileGeom g, QuantileLevels ql) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (e >= chw) return;
    const int x = (int)(e % (unsigned)g.W);
    const unsigned long long cy = e / (unsigned)g.W;
    const int y = (int)(cy % (unsigned)g.H), c = (int)(cy / (unsigned)g.H);
    int ky0, ky1, kx0, kx1;
    tile_cover(y, g.H, g.th, g.ny, &ky0, &ky1);
    tile_cover(x, g.W, g.tw, g.nx, &kx0, &kx1);
    const size_t tile_plane = (size_t)g.th * g.tw, K = (size_t)g.ny * g.nx;
    const size_t member_stride = (size_t)B * K * g.C * tile_plane;             // tile block m * B + b: m * member_stride further on
    for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) {
        double num[KP], den = 0.0;
#pragma unroll
        for (int m = 0; m < KP; ++m) num[m] = 0.0;
        for (int ky = ky0; ky <= ky1; ++ky) {
            const int ry = y - tile_origin(ky, g.H, g.th, g.ny);
            const int wy = tile_window(ry, g.th, g.oy);
            for (int kx = kx0; kx <= kx1; ++kx) {
                const int rx = x - tile_origin(kx, g.W, g.tw, g.nx);
                const double w = (double)(wy * tile_window(rx, g.tw, g.ox));
                const float* src = tiles + ((b * K + (size_t)ky * g.nx + kx) * g.C + c) * tile_plane + (size_t)ry * g.tw + rx;
#pragma unroll
                for (int m = 0; m < KP; ++m)
                    if (m < M) num[m] = add_rn64(num[m], mul_rn64(w, (double)src[(size_t)m * member_stride]));
                den = add_rn64(den, w);
            }
        }
        uint32_t key[KP];
        bool has_nan = false;
#pragma unroll
        for (int m = 0; m < KP; ++m) {
            if (m < M) {
                const uint32_t bits = __float_as_uint(__double2float_rn(__ddiv_rn(num[m], den)));
                key[m] = order_key(bits);
                has_nan = has_nan || is_nan_bits(bits);
            } else {
                key[m] = ORDER_KEY_PAD;
            }
        }
        sort_keys<KP>(key);
        float* dst = out + b * (size_t)ql.nq * chw + e;
        for (int i = 0; i < ql.nq; ++i) dst[(size_t)i * chw] = quantile_of_sorted<KP>(key, quantile_pos(ql.q[i], M), M, has_nan);
    }
}

hipError_t tile_blend_quantiles_launch(const float* tiles, int B, int M, const TileGeom& g, const QuantileLevels& ql, float* out, hipStream_t s) {
    dim3 grid;
    if (!tile_blend_geom_ok(B, g, &grid) || M < 1 || M > QUANTILE_MAX_MEMBERS || !tiles || !out || !quantile_levels_ok(ql)) return hipErrorInvalidValue;
    if (!tile_blocks_ok(B, M, g)) return hipErrorInvalidValue;
#define MIDD_TBQ(N) hipLaunchKernelGGL(tile_blend_quantiles_kernel<N>, grid, dim3(256), 0, s, tiles, out, B, M, g, ql)
    if (M <= 2) MIDD_TBQ(2);
    else if (M <= 4) MIDD_TBQ(4);
    else if (M <= 8) MIDD_TBQ(8);
    else if (M <= 16) MIDD_TBQ(16);
    else if (M <= 32) MIDD_TBQ(32);
    else MIDD_TBQ(64);
#undef MIDD_TBQ
    return hipGetLastError();
}

}  // namespace midd
