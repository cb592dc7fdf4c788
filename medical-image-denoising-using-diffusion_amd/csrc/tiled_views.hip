// The tiled self-ensemble (mi_denoise_tiled_self_ensemble): flip / rotate views of images of any size >= the tile.  HBM-bound
// gathers, all of it data movement, the blend's fixed double arithmetic and per-pixel statistics.
//
//   plane_view_kernel                 : view(images, g) of H x W planes, H != W included: the viewed batch of one round
//   tile_blend_unview_reduce_kernel   : every view's tiles blended in the VIEW's frame, turned back, and mean / std over them
//   tile_blend_unview_quantiles_kernel: the same gather, and per-pixel quantiles over them
#include "midd_internal.h"
#include "tile_geometry.h"
#include "quantile_common.h"
#include <type_traits>

namespace midd {

// THE GEOMETRY IS FIXED (include/midd.h): view code g = 4 t + 2 fy + fx on the last two axes of a [C][H][W] image,
//   t = 0:  view(x)[p][q] = x[fy ? H-1-p : p][fx ? W-1-q : q]                   (Hv x Wv = H x W; its own inverse)
//   t = 1:  view(x)[p][q] = x[fx ? H-1-q : q][fy ? W-1-p : p]                   (Hv x Wv = W x H)
//           unview(v)[y][x] = v[fy ? W-1-x : x][fx ? H-1-y : y]
// and view k's tiles are the tiles of the VIEWED image: the tile geometry of (Hv, Wv) -- with t = 1 the host accepts square
// tiles and overlaps only (th == tw, oy == ox), so that frame has nx x ny tiles of the same shape.
// A workgroup of 256 threads owns a TV_T x TV_T (32 x 32) patch of one [H][W] plane of the destination; thread (r = tid / 8,
// c = tid % 8) owns the four neighbouring pixels (y0 + r, x0 + 4 c ..+3), as in dihedral.hip.  Where the source is transposed the
// pixel to the right is the pixel BELOW in the source, so the workgroup's threads are re-assigned: thread (r, c) forms the four
// values of destination pixels (y0 + 4 c ..+3, x0 + r) -- a run of one source row -- and hands them over through an LDS patch
// [x - x0][y - y0] of pitch 33 words: the stores (bank r + 4 c + j) and the loads (bank 4 c + j + r) of a 32-lane group hit 32
// different banks.  One barrier, then every thread picks its own pixels up.
constexpr int TV_T = 32, TV_PITCH = TV_T + 1, TV_PATCH = TV_T * TV_PITCH;
// Pointers that pass through a register pin (thread_pointer, gather_members) are typed as GLOBAL memory: an address that went
// through an asm operand has lost the address space the compiler infers for kernel arguments, and would be accessed with flat_*
// instructions otherwise.
typedef float __attribute__((address_space(1))) gfloat;
typedef f32x4 __attribute__((address_space(1))) gf32x4;

struct ViewPatch { int y0, x0, c; };
__device__ __forceinline__ ViewPatch view_patch(int H, int W) {
    const unsigned px = (unsigned)(W + TV_T - 1) / TV_T, py = (unsigned)(H + TV_T - 1) / TV_T;
    const unsigned ix = blockIdx.x % px, rest = blockIdx.x / px;
    return ViewPatch{(int)(rest % py) * TV_T, (int)ix * TV_T, (int)(rest / py)};
}

// o: the address of the quad's first pixel, column x of a row of W floats
template <class P>
__device__ __forceinline__ void store_quad(P* o, int W, int x, int vec, const float (&v)[4]) {
    if (vec) {
        if constexpr (std::is_same<P, gfloat>::value) *(gf32x4*)o = (f32x4){v[0], v[1], v[2], v[3]};
        else *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (x + j < W) o[j] = v[j];
    }
}

// A thread's own output address, formed BEFORE the gather and pinned into vector registers there: the base pointers and strides it
// is made of are scalar registers that would otherwise stay live across the gather, which needs every one of them itself.
__device__ __forceinline__ gfloat* thread_pointer(float* base, size_t offset) {
    uintptr_t a = base ? reinterpret_cast<uintptr_t>(base + offset) : 0;
    asm volatile("" : "+v"(a));
    return (gfloat*)a;
}

__device__ __forceinline__ void patch_put(float* patch, int rows, int cols, const float (&v)[4]) {
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    if (r < rows) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (c4 + j < cols) patch[r * TV_PITCH + c4 + j] = v[j];
    }
}

__device__ __forceinline__ void patch_get(const float* patch, float (&out)[4]) {
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = patch[(c4 + j) * TV_PITCH + r];     // (words outside the plane hold stale LDS: never stored to memory)
}

// ------------------------------------------------------------------------------ the fill: one view of a batch of planes
// out[j] <- src[row][rev ? L-1-(q+j) : q+j], j = 0..3 with q + j < L (the others keep their value), of a row of L floats
__device__ __forceinline__ void row_quad(const float* __restrict__ row, int L, int q, bool rev, int vec, float (&out)[4]) {
    if (vec) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + (rev ? L - 4 - q : q));
        out[0] = rev ? v.w : v.x; out[1] = rev ? v.z : v.y; out[2] = rev ? v.y : v.z; out[3] = rev ? v.x : v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q + j < L) out[j] = row[rev ? L - 1 - (q + j) : q + j];
    }
}

// dst [B][C][Hv][Wv] <- view(images [B][C][H][W], code): bit copies.  grid (patches of a destination plane * C, B); the code is a
// launch constant.  vload: source rows move as 16 bytes (W % 4 == 0, images 16-byte aligned); vstore: Wv % 4 == 0, dst aligned
__global__ __launch_bounds__(256)
void plane_view_kernel(const float* __restrict__ images, float* __restrict__ dst, int code, int C, int H, int W, int vload, int vstore) {
    __shared__ float patch[TV_PATCH];
    const bool t = code & 4, fy = code & 2, fx = code & 1;
    const int Hv = t ? W : H, Wv = t ? H : W;
    const ViewPatch vp = view_patch(Hv, Wv);
    const size_t plane = (size_t)H * W, at = ((size_t)blockIdx.y * C + vp.c) * plane;
    const float* src = images + at;
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    const int p = vp.y0 + r, q = vp.x0 + c4;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (t) {                                                  // dst[p][q] = src[fx ? H-1-q : q][fy ? W-1-p : p]: source row of q0 + r, columns of p0 + 4 c ..
        const int sq = vp.x0 + r, sp = vp.y0 + c4;
        if (sq < Wv && sp < Hv) row_quad(src + (size_t)(fx ? H - 1 - sq : sq) * W, W, sp, fy, vload, x);
        patch_put(patch, Wv - vp.x0, Hv - vp.y0, x);
        __syncthreads();
        patch_get(patch, x);
    } else if (p < Hv && q < Wv) {
        row_quad(src + (size_t)(fy ? H - 1 - p : p) * W, W, q, fx, vload, x);
    }
    if (p < Hv && q < Wv) store_quad(dst + at + (size_t)p * Wv + q, Wv, q, vstore, x);
}

static bool view_planes_ok(int C, int H, int W, unsigned* grid_x) {
    if (C < 1 || H < 1 || W < 1 || (unsigned long long)C * H * W >= (1ull << 32)) return false;
    const unsigned long long blocks = (unsigned long long)((H + TV_T - 1) / TV_T) * ((W + TV_T - 1) / TV_T) * C;      // (the same count in either frame)
    if (blocks > 2147483647ull) return false;
    *grid_x = (unsigned)blocks;
    return true;
}

hipError_t plane_view_launch(const float* images, float* dst, int code, int B, int C, int H, int W, hipStream_t s) {
    unsigned gx = 0;
    if (!view_planes_ok(C, H, W, &gx) || code < 0 || code > 7 || B < 1 || B > 65535 || !images || !dst) return hipErrorInvalidValue;
    const int Wv = (code & 4) ? H : W;
    const int vload = (W % 4 == 0 && aligned16(images)) ? 1 : 0, vstore = (Wv % 4 == 0 && aligned16(dst)) ? 1 : 0;
    hipLaunchKernelGGL(plane_view_kernel, dim3(gx, B), dim3(256), 0, s, images, dst, code, C, H, W, vload, vstore);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ blend in a view's frame
// The frame of one view: its image is Hf x Wf and is cut into ny x nx tiles of th x tw (tile_geometry.h)
struct TileFrame { int Hf, Wf, ny, nx; };
__device__ __forceinline__ TileFrame tile_frame(const TileGeom& g, bool t) {
    return t ? TileFrame{g.W, g.H, g.nx, g.ny} : TileFrame{g.H, g.W, g.ny, g.nx};
}

// v[i] <- mi_tile_blend's pixel (c, p, q + i), i = 0..3, of one image's tiles [ny*nx][C][th][tw] in the frame f (tiles_c: channel
// c of the image's first tile), for the pixels with 0 <= q + i < Wf (the others keep their value); 0 <= p < Hf and at least one
// of the four lies inside.  THE ARITHMETIC IS tile_blend_kernel's, per pixel: the tiles
// that cover it in ascending (ky, kx), num += (double)(wy * wx) * (double)v, den += (double)(wy * wx), (float)(num / den), every
// operation rounded on its own.  The four pixels share the row cover; the column tiles walked are those from the first that
// covers the leftmost pixel to the last that covers the rightmost (origins ascend, so every tile between covers one of them),
// and a pixel takes part in a tile only when it lies inside: each pixel meets exactly its own tiles, in its own order.  A tile
// row moves as 16 bytes when all four pixels lie in the tile and the address allows it (vload: tw % 4 == 0, tiles 16-byte
// aligned; then rx % 4 == 0 decides), else as dwords -- the same values.
__device__ __forceinline__ void blend_quad(const gfloat* tiles_c, const TileGeom& g, const TileFrame& f, int p, int q,
                                           int vload, float (&v)[4]) {
    const int qa = q < 0 ? 0 : q, qb = q + 3 >= f.Wf ? f.Wf - 1 : q + 3;
    int ky0, ky1, kx0, kx1, unused;
    tile_cover(p, f.Hf, g.th, f.ny, &ky0, &ky1);
    tile_cover(qa, f.Wf, g.tw, f.nx, &kx0, &unused);
    tile_cover(qb, f.Wf, g.tw, f.nx, &unused, &kx1);
    const size_t tile_plane = (size_t)g.th * g.tw;
    double num[4] = {0.0, 0.0, 0.0, 0.0}, den[4] = {0.0, 0.0, 0.0, 0.0};
    for (int ky = ky0; ky <= ky1; ++ky) {
        const int ry = p - tile_origin(ky, f.Hf, g.th, f.ny);
        const int wy = tile_window(ry, g.th, g.oy);
        for (int kx = kx0; kx <= kx1; ++kx) {
            const int rx = q - tile_origin(kx, f.Wf, g.tw, f.nx);               // of pixel 0; pixel i: rx + i
            const gfloat* src = tiles_c + ((size_t)ky * f.nx + kx) * g.C * tile_plane + (size_t)ry * g.tw;
            float t[4] = {0.f, 0.f, 0.f, 0.f};
            if (vload && rx >= 0 && rx + 3 < g.tw && (rx & 3) == 0) {
                const f32x4 r = *(const gf32x4*)(src + rx);
                t[0] = r.x; t[1] = r.y; t[2] = r.z; t[3] = r.w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (rx + i >= 0 && rx + i < g.tw) t[i] = src[rx + i];
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (rx + i >= 0 && rx + i < g.tw) {
                    const double w = (double)(wy * tile_window(rx + i, g.tw, g.ox));
                    num[i] = add_rn64(num[i], mul_rn64(w, (double)t[i]));
                    den[i] = add_rn64(den[i], w);
                }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
        if (q + i >= 0 && q + i < f.Wf) v[i] = __double2float_rn(__ddiv_rn(num[i], den[i]));
}

// The members of a thread's four pixels: x[k][j] = unview(mi_tile_blend(tiles[k][b]) in view k's frame, code[k]) at pixel
// (y, x0 + 4 c + j), k = 0 .. n-1 in list order, in registers.  A pixel's blend is a function of the pixel alone, so which thread
// forms it does not change a bit.  The loop over the views is ROLLED -- one copy of the blend in the instruction stream, the view
// codes packed into one word (4 bits each) -- and view k's quad lands in x[k] through an unrolled chain of selects over the NV
// constant indices: the member array is never indexed by a run-time value and stays in registers.  TR (some view of the list
// transposes): every transposing view gets an LDS patch of its own (at most four codes transpose), all are staged, ONE barrier,
// then every thread picks its pixels up.  !TR: no LDS, no barrier.
template <bool TR, int NV>
__device__ __forceinline__ void gather_members(const float* __restrict__ tiles, size_t view_stride, const DihedralViews& dv, const TileGeom& g,
                                               const ViewPatch& vp, int vload, float* patches, float (&x)[NV][4]) {
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    const int H = g.H, W = g.W, n = dv.n < NV ? dv.n : NV;
    uint32_t codes = 0;
#pragma unroll
    for (int k = 0; k < NV; ++k) codes |= (uint32_t)(dv.code[k] & 7) << (4 * k);
    // (the walk's base address and stride are uniform, but every load address is per thread anyway: kept in vector registers, they
    // leave the scalar ones to the blend's loop state)
    uintptr_t tiles_a = reinterpret_cast<uintptr_t>(tiles + (size_t)vp.c * g.th * g.tw);
    asm volatile("" : "+v"(tiles_a), "+v"(view_stride));
    const gfloat* tiles_c = (const gfloat*)tiles_a;
#pragma unroll
    for (int k = 0; k < NV; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[k][j] = 0.f;
    }
    // TR: two walks over the list in ONE loop, so that the blend exists once in the instruction stream: walk 0 stages the
    // transposing views (this thread forms output pixels (y0 + 4 c ..+3, x0 + r): a run of one row of the W x H frame), the
    // barrier, walk 1 blends the others in place and picks the staged ones up.  The trip count is uniform in the workgroup.
    const int walks = TR ? 2 : 1;
    int slot = 0;
#pragma unroll 1
    for (int it = 0; it < walks * n; ++it) {
        const bool stage = TR && it < n;
        if (TR && it == n) { __syncthreads(); slot = 0; }
        const int k = (TR && it >= n) ? it - n : it;
        const uint32_t code = (codes >> (4 * k)) & 7;
        const bool t = TR && (code & 4), fy = code & 2, fx = code & 1;
        float o[4] = {0.f, 0.f, 0.f, 0.f};
        if (stage != t) {
            if (stage) continue;                                               // a view read in place: walk 1
            patch_get(patches + slot * TV_PATCH, o);                           // a staged view
            ++slot;
        } else {
            const TileFrame f = tile_frame(g, t);
            const int oy = vp.y0 + (t ? c4 : r), ox = vp.x0 + (t ? r : c4);    // first output pixel of the quad this thread forms: a run of rows (t) or of columns
            const int p = t ? (fy ? W - 1 - ox : ox) : (fy ? H - 1 - oy : oy);
            const int q = t ? (fx ? H - 4 - oy : oy) : (fx ? W - 4 - ox : ox);
            float v[4] = {0.f, 0.f, 0.f, 0.f};
            if (oy < H && ox < W) blend_quad(tiles_c + k * view_stride, g, f, p, q, vload, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) o[j] = fx ? v[3 - j] : v[j];
            if (t) {
                patch_put(patches + slot * TV_PATCH, W - vp.x0, H - vp.y0, o);
                ++slot;
                continue;
            }
        }
#pragma unroll
        for (int kk = 0; kk < NV; ++kk) {
#pragma unroll
            for (int j = 0; j < 4; ++j) x[kk][j] = (kk == k) ? o[j] : x[kk][j];
        }
    }
}

// The final launch of mi_denoise_tiled_self_ensemble: tiles [G][B][K][C][th][tw], the tile outputs of every view in that view's
// frame, in run order -> mean / unbiased std [B][C][H][W] over the G views blended and turned back and, if asked for, those
// aligned members [B][G][C][H][W].  THE ARITHMETIC IS FIXED (include/midd.h: mi_tile_blend_unview_reduce): the gather above, then
// exactly ensemble_reduce_kernel's sums over x_0 .. x_{G-1} in list order -- mi_tile_blend per view, unview, mi_ensemble_reduce,
// bit for bit, with or without `samples`.  G <= 8: the members stay in registers, nothing is blended twice.
// grid (patches of a plane * C, B)
template <bool TR>
__global__ __launch_bounds__(256)
void tile_blend_unview_reduce_kernel(const float* __restrict__ tiles, float* __restrict__ mean, float* __restrict__ stdv, float* __restrict__ samples,
                                     DihedralViews dv, TileGeom g, int B, int vload, int vstore) {
    __shared__ float patches[TR ? 4 * TV_PATCH : 1];
    const int H = g.H, W = g.W, G = dv.n;
    const ViewPatch vp = view_patch(H, W);
    const size_t b = blockIdx.y, plane = (size_t)H * W, chw = (size_t)g.C * plane;
    const size_t image_tiles = (size_t)g.ny * g.nx * g.C * g.th * g.tw;        // the tiles of one image of one view
    const int y = vp.y0 + (threadIdx.x >> 3), x0 = vp.x0 + (threadIdx.x & 7) * 4;
    const size_t px = (size_t)vp.c * plane + (size_t)y * W + x0;                // the quad inside a [C][H][W] block (used only when inside)
    gfloat* mean_p = thread_pointer(mean, b * chw + px);
    gfloat* std_p = thread_pointer(stdv, b * chw + px);
    gfloat* samples_p = thread_pointer(samples, b * G * chw + px);
    float x[DIHEDRAL_MAX_VIEWS][4];
    gather_members<TR, DIHEDRAL_MAX_VIEWS>(tiles + b * image_tiles, (size_t)B * image_tiles, dv, g, vp, vload, patches, x);
    if (y >= H || x0 >= W) return;                           // (after the barrier)
    double sum[4], m64[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] = 0.0;
#pragma unroll
    for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k)
        if (k < G) {
            if (samples_p) store_quad(samples_p + (size_t)k * chw, W, x0, vstore, x[k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) sum[j] = add_rn64(sum[j], (double)x[k][j]);
        }
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { m64[j] = __ddiv_rn(sum[j], (double)G); out[j] = __double2float_rn(m64[j]); }
    if (mean_p) store_quad(mean_p, W, x0, vstore, out);
    if (std_p) {
        double dev[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) dev[j] = 0.0;
#pragma unroll
        for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k)
            if (k < G) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const double d = sub_rn64((double)x[k][j], m64[j]); dev[j] = add_rn64(dev[j], mul_rn64(d, d)); }
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = __double2float_rn(__dsqrt_rn(__ddiv_rn(dev[j], (double)(G - 1))));
        store_quad(std_p, W, x0, vstore, out);
    }
}

// What both launches refuse: a bad view list, a transposing code with a non-square tile or overlap, a geometry the blend kernels
// refuse, more than 65535 images (grid.y), tile blocks beyond an int
static bool unview_launch_ok(int B, const DihedralViews& dv, const TileGeom& g, unsigned* grid_x, bool* transposes) {
    if (dv.n < 1 || dv.n > DIHEDRAL_MAX_VIEWS || B < 1 || B > 65535) return false;
    *transposes = false;
    for (int k = 0; k < dv.n; ++k) {
        if (dv.code[k] > 7) return false;
        if (dv.code[k] & 4) *transposes = true;
    }
    if (*transposes && (g.th != g.tw || g.oy != g.ox)) return false;
    if (g.ny < 1 || g.nx < 1 || g.th < 1 || g.tw < 1 || g.th > g.H || g.tw > g.W || g.oy < 0 || g.ox < 0 ||
        (long long)g.oy + 1 > 46340 || (long long)g.ox + 1 > 46340) return false;
    if (g.ny != tile_count(g.H, g.th, g.oy) || g.nx != tile_count(g.W, g.tw, g.ox)) return false;
    if ((long long)B * g.ny * g.nx * dv.n > 2147483647ll) return false;
    return view_planes_ok(g.C, g.H, g.W, grid_x);
}

hipError_t tile_blend_unview_reduce_launch(const float* tiles, int B, const DihedralViews& dv, const TileGeom& g,
                                           float* mean, float* stdv, float* samples, hipStream_t s) {
    unsigned gx = 0;
    bool tr = false;
    if (!unview_launch_ok(B, dv, g, &gx, &tr) || !tiles || (!mean && !stdv && !samples) || (stdv && dv.n < 2)) return hipErrorInvalidValue;
    const int vload = (g.tw % 4 == 0 && aligned16(tiles)) ? 1 : 0;
    const int vstore = (g.W % 4 == 0 && aligned16(mean) && aligned16(stdv) && aligned16(samples)) ? 1 : 0;
    if (tr)
        hipLaunchKernelGGL(tile_blend_unview_reduce_kernel<true>, dim3(gx, B), dim3(256), 0, s, tiles, mean, stdv, samples, dv, g, B, vload, vstore);
    else
        hipLaunchKernelGGL(tile_blend_unview_reduce_kernel<false>, dim3(gx, B), dim3(256), 0, s, tiles, mean, stdv, samples, dv, g, B, vload, vstore);
    return hipGetLastError();
}

// tiles as above -> out [B][nq][C][H][W]: the gather above, every member formed once, then the sort and the interpolation of
// ensemble_quantiles_kernel over x_0 .. x_{G-1}: mi_ensemble_quantiles of the aligned members, bit for bit, which never exist in
// memory.  KP in {2, 4, 8} >= G: KP members and KP keys per pixel, all at constant register indices.  grid as above
template <int KP, bool TR>
__global__ __launch_bounds__(256)
void tile_blend_unview_quantiles_kernel(const float* __restrict__ tiles, float* __restrict__ out, DihedralViews dv, TileGeom g, QuantileLevels ql,
                                        int B, int vload, int vstore) {
    __shared__ float patches[TR ? (KP < 4 ? KP : 4) * TV_PATCH : 1];
    const int H = g.H, W = g.W, G = dv.n;
    const ViewPatch vp = view_patch(H, W);
    const size_t b = blockIdx.y, plane = (size_t)H * W, chw = (size_t)g.C * plane;
    const size_t image_tiles = (size_t)g.ny * g.nx * g.C * g.th * g.tw;
    const int y = vp.y0 + (threadIdx.x >> 3), x0 = vp.x0 + (threadIdx.x & 7) * 4;
    gfloat* dst = thread_pointer(out, b * (size_t)ql.nq * chw + (size_t)vp.c * plane + (size_t)y * W + x0);      // (used only when inside)
    float x[KP][4];
    gather_members<TR, KP>(tiles + b * image_tiles, (size_t)B * image_tiles, dv, g, vp, vload, patches, x);
    if (y >= H || x0 >= W) return;                           // (after the barrier)
    uint32_t key[4][KP];
    bool has_nan[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        has_nan[j] = false;
#pragma unroll
        for (int k = 0; k < KP; ++k) {
            const uint32_t bits = __float_as_uint(x[k][j]);
            key[j][k] = (k < G) ? order_key(bits) : ORDER_KEY_PAD;
            has_nan[j] = has_nan[j] || (k < G && is_nan_bits(bits));
        }
        sort_keys<KP>(key[j]);
    }
    for (int i = 0; i < ql.nq; ++i) {
        const QuantilePos pos = quantile_pos(ql.q[i], G);
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = quantile_of_sorted<KP>(key[j], pos, G, has_nan[j]);
        store_quad(dst + (size_t)i * chw, W, x0, vstore, r);
    }
}

hipError_t tile_blend_unview_quantiles_launch(const float* tiles, int B, const DihedralViews& dv, const TileGeom& g,
                                              const QuantileLevels& ql, float* out, hipStream_t s) {
    unsigned gx = 0;
    bool tr = false;
    if (!unview_launch_ok(B, dv, g, &gx, &tr) || !tiles || !out || !quantile_levels_ok(ql)) return hipErrorInvalidValue;
    const int vload = (g.tw % 4 == 0 && aligned16(tiles)) ? 1 : 0;
    const int vstore = (g.W % 4 == 0 && aligned16(out)) ? 1 : 0;
#define MIDD_TBUQ(N, T) hipLaunchKernelGGL((tile_blend_unview_quantiles_kernel<N, T>), dim3(gx, B), dim3(256), 0, s, tiles, out, dv, g, ql, B, vload, vstore)
    if (dv.n <= 2) { if (tr) MIDD_TBUQ(2, true); else MIDD_TBUQ(2, false); }
    else if (dv.n <= 4) { if (tr) MIDD_TBUQ(4, true); else MIDD_TBUQ(4, false); }
    else { if (tr) MIDD_TBUQ(8, true); else MIDD_TBUQ(8, false); }
#undef MIDD_TBUQ
    return hipGetLastError();
}

}  // namespace midd
