// The consensus of overlapping tiles (include/midd.h: mi_tile_consensus, THE CONSENSUS): every tile element that lies over an
// image pixel is replaced by the blend of all the elements over that pixel, in place, in ONE pass -- what mi_denoise_tiled_fused
// runs after every sampler step so that neighbouring tiles enter the next forward with the same values wherever they share pixels.
//
//   tile_consensus_kernel : tiles [B][ny*nx][C][th][tw] -> themselves (and, if asked for, the blended image [B][C][H][W])
#include "midd_internal.h"
#include "tile_geometry.h"
#include "pointwise_common.h"

namespace midd {

// A thread owns ONE image pixel (V = 1) or FOUR neighbouring pixels of one image row (V = 4), finds the tiles that cover it from
// the origin formula exactly as tile_blend_kernel does (tile_cover; the loops do not rely on "at most three per axis") and walks
// them twice in ascending (ky, kx): once to READ the covering elements and form
//   num += (double)(wy * wx) * (double)v;   den += (double)(wy * wx);   r = (float)(num / den)
// -- THE ARITHMETIC of mi_tile_blend, in double, every operation rounded on its own, no FMA, one rounding to fp32 -- and once to
// WRITE r to every covering element; r also goes to `image` when there is one.  So the tiles afterwards are
// mi_tile_extract(mi_tile_blend(tiles)) and the image is mi_tile_blend(tiles), bit for bit, with cover reads and cover (+ 1)
// writes per pixel and no image-sized temporary.
//
// WHY IN PLACE IS SAFE.  A tile element lies over exactly one image pixel (b, c, y0 + ry, x0 + rx), and a pixel is owned by
// exactly one thread of the launch.  The thread that owns a pixel has read ALL of its covering elements before it writes ANY of
// them (r depends on every load), and no other thread ever touches those elements: there is no read of another thread's write,
// whatever the grid.  No atomics, no LDS, no scratch (the walk is repeated, nothing is kept per tile).
//
// V = 4 (W % 4 == 0, tw % 4 == 0, tiles and image 16-byte aligned: the launch decides): a thread's four pixels x .. x + 3 take
// the 16-byte path when they share their cover set on the x axis and sit at a multiple of four inside every covering tile --
// then every covering run of four elements is one aligned 16-byte load and store; else the thread walks its four pixels one by
// one on the dword path.  The value of a pixel is the same function of the same loads either way: the bits do not depend on the
// path, the grid or the alignment.
// grid (chunks of 256 threads over C * H * W / V, images -- folded over grid.y when B > 65535)
__device__ __forceinline__ size_t consensus_elem(const TileGeom& g, size_t b, int ky, int kx, int c, int ry, int rx) {
    return (((b * ((size_t)g.ny * g.nx) + (size_t)ky * g.nx + kx) * g.C + c) * g.th + ry) * (size_t)g.tw + rx;
}

// one pixel on the dword path: -> its value, written to every covering element
__device__ __forceinline__ float consensus_pixel(float* tiles, const TileGeom& g, size_t b, int c, int y, int x, int ky0, int ky1) {
    int kx0, kx1;
    tile_cover(x, g.W, g.tw, g.nx, &kx0, &kx1);
    double num = 0.0, den = 0.0;
    for (int ky = ky0; ky <= ky1; ++ky) {
        const int ry = y - tile_origin(ky, g.H, g.th, g.ny);
        const int wy = tile_window(ry, g.th, g.oy);
        for (int kx = kx0; kx <= kx1; ++kx) {
            const int rx = x - tile_origin(kx, g.W, g.tw, g.nx);
            const double w = (double)(wy * tile_window(rx, g.tw, g.ox));
            const float v = tiles[consensus_elem(g, b, ky, kx, c, ry, rx)];
            num = add_rn64(num, mul_rn64(w, (double)v));
            den = add_rn64(den, w);
        }
    }
    const float r = __double2float_rn(__ddiv_rn(num, den));
    for (int ky = ky0; ky <= ky1; ++ky) {
        const int ry = y - tile_origin(ky, g.H, g.th, g.ny);
        for (int kx = kx0; kx <= kx1; ++kx)
            tiles[consensus_elem(g, b, ky, kx, c, ry, x - tile_origin(kx, g.W, g.tw, g.nx))] = r;
    }
    return r;
}

template <int V>
__global__ __launch_bounds__(256)
void tile_consensus_kernel(float* tiles, float* __restrict__ image, int B, TileGeom g) {
    const unsigned long long e = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * V;
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (e >= chw) return;                                              // (V == 4: chw % 4 == 0, so e + 3 < chw)
    const int x = (int)(e % (unsigned)g.W);
    const unsigned long long cy = e / (unsigned)g.W;
    const int y = (int)(cy % (unsigned)g.H), c = (int)(cy / (unsigned)g.H);
    int ky0, ky1;
    tile_cover(y, g.H, g.th, g.ny, &ky0, &ky1);
    if constexpr (V == 4) {
        int kx0, kx1, lx0, lx1;
        tile_cover(x, g.W, g.tw, g.nx, &kx0, &kx1);
        tile_cover(x + 3, g.W, g.tw, g.nx, &lx0, &lx1);                 // (W % 4 == 0: x + 3 is in the same row)
        bool quad = kx0 == lx0 && kx1 == lx1;                           // first and last are monotone in x: x + 1, x + 2 agree too
        for (int kx = kx0; kx <= kx1; ++kx) quad = quad && ((x - tile_origin(kx, g.W, g.tw, g.nx)) & 3) == 0;
        if (quad) {
            for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) {
                double num[4] = {0.0, 0.0, 0.0, 0.0}, den[4] = {0.0, 0.0, 0.0, 0.0};
                for (int ky = ky0; ky <= ky1; ++ky) {
                    const int ry = y - tile_origin(ky, g.H, g.th, g.ny);
                    const int wy = tile_window(ry, g.th, g.oy);
                    for (int kx = kx0; kx <= kx1; ++kx) {
                        const int rx = x - tile_origin(kx, g.W, g.tw, g.nx);
                        const f32x4 v = *reinterpret_cast<const f32x4*>(tiles + consensus_elem(g, b, ky, kx, c, ry, rx));
#pragma unroll
                        for (int j = 0; j < 4; ++j) {
                            const double w = (double)(wy * tile_window(rx + j, g.tw, g.ox));
                            num[j] = add_rn64(num[j], mul_rn64(w, (double)v[j]));
                            den[j] = add_rn64(den[j], w);
                        }
                    }
                }
                f32x4 r;
#pragma unroll
                for (int j = 0; j < 4; ++j) r[j] = __double2float_rn(__ddiv_rn(num[j], den[j]));
                for (int ky = ky0; ky <= ky1; ++ky) {
                    const int ry = y - tile_origin(ky, g.H, g.th, g.ny);
                    for (int kx = kx0; kx <= kx1; ++kx)
                        *reinterpret_cast<f32x4*>(tiles + consensus_elem(g, b, ky, kx, c, ry, x - tile_origin(kx, g.W, g.tw, g.nx))) = r;
                }
                if (image) *reinterpret_cast<f32x4*>(image + b * chw + e) = r;
            }
            return;
        }
    }
    for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) {
#pragma unroll
        for (int j = 0; j < V; ++j) {
            const float r = consensus_pixel(tiles, g, b, c, y, x + j, ky0, ky1);
            if (image) image[b * chw + e + j] = r;
        }
    }
}

// What the launch refuses in (B, g) is what every blend launch refuses (tiles.hip: tile_blend_geom_ok -- a tile outside the image,
// chw >= 2^32, a window product that does not fit an int), restated here so that tiles.hip stays the unit it is.
hipError_t tile_consensus_launch(float* tiles, float* image, int B, const TileGeom& g, hipStream_t s) {
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (!tiles || B < 1 || g.C < 1 || g.ny < 1 || g.nx < 1 || g.th < 1 || g.tw < 1 || g.th > g.H || g.tw > g.W || chw >= (1ull << 32) ||
        g.oy < 0 || g.ox < 0 || (long long)g.oy + 1 > 46340 || (long long)g.ox + 1 > 46340) return hipErrorInvalidValue;
    const unsigned by = B < 65535 ? B : 65535;
    if (g.W % 4 == 0 && g.tw % 4 == 0 && aligned16(tiles) && aligned16(image))          // (a null image is "aligned": it is not written)
        hipLaunchKernelGGL(tile_consensus_kernel<4>, dim3((unsigned)((chw / 4 + 255) / 256), by), dim3(256), 0, s, tiles, image, B, g);
    else
        hipLaunchKernelGGL(tile_consensus_kernel<1>, dim3((unsigned)((chw + 255) / 256), by), dim3(256), 0, s, tiles, image, B, g);
    return hipGetLastError();
}

}  // namespace midd
