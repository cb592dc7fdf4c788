// The geometric self-ensemble (mi_denoise_self_ensemble): HBM-bound gathers, all of it data movement and per-pixel statistics.
//
//   dihedral_views_kernel     : the flip / rotate views of the images, the sampler's virtual samples
//   dihedral_reduce_kernel    : the views' outputs turned back, and mean / std over them
//   dihedral_quantiles_kernel : the same gather, and per-pixel quantiles over them
#include "midd_internal.h"
#include "quantile_common.h"

namespace midd {

// ------------------------------------------------------------------------------ geometric self-ensemble: the 8 flip / rotate views
// THE GEOMETRY IS FIXED (include/midd.h): view code g = 4 t + 2 fy + fx on the last two axes of a [C][H][W] image,
//   non-transposing (t = 0):  view(x)[p][q] = x[fy ? H-1-p : p][fx ? W-1-q : q]     and unview is the same map (an involution)
//   transposing (t = 1, H == W == N):  view(x)[p][q] = x[fx ? N-1-q : q][fy ? N-1-p : p],  unview(v)[p][q] = v[fy ? N-1-q : q][fx ? N-1-p : p]
// so every direction is ONE gather  dst[p][q] = src[rr ? .. q : q][rc ? .. p : p]  (transposing) or  src[rr ? .. p][rc ? .. q]  (not),
// with (rr, rc) = (fy, fx) except for the transposing view() itself, where they swap.  All of it is data movement: bit copies.
// A workgroup of 256 threads owns a DH_T x DH_T (32 x 32) tile of one [H][W] plane of the destination; thread (r = tid / 8,
// c = tid % 8) owns the four neighbouring pixels (p0 + r, q0 + 4 c ..+3).  Not transposing, a thread's quad is a quad of one source
// row, read in place (reversed inside the quad when rc): no LDS.  Transposing, the quad is a piece of a source COLUMN, one float per
// 4 N bytes: the workgroup reads the transposed source tile row by row instead (thread (r, c): source row of q0 + r, the quad of
// columns of p0 + 4 c ..+3: 128 contiguous bytes per 8 lanes, whole lines) into an LDS patch [q - q0][p - p0] of pitch 33 words --
// the reversals are applied on the way in, so the patch is in destination coordinates -- and after one barrier reads its pixels
// from patch[4 c + j][r]: with pitch 33 both the stores (bank r + 4 c + j) and the loads (bank 4 c + j + r) of a 32-lane group hit 32
// different banks.  `vec`: the quads move as 16 bytes (W % 4 == 0, every pointer 16-byte aligned: then a quad never crosses the
// right edge and every quad start, reversed or not, is a multiple of 4); else dword by dword with bounds checks -- the same values.
constexpr int DH_T = 32, DH_PITCH = DH_T + 1, DH_PATCH = DH_T * DH_PITCH;

struct DihedralTile { int p0, q0, c; };
__device__ __forceinline__ DihedralTile dihedral_tile(int H, int W) {
    const unsigned tiles_q = (unsigned)(W + DH_T - 1) / DH_T, tiles_p = (unsigned)(H + DH_T - 1) / DH_T;
    const unsigned tq = blockIdx.x % tiles_q, rest = blockIdx.x / tiles_q;
    return DihedralTile{(int)(rest % tiles_p) * DH_T, (int)tq * DH_T, (int)(rest / tiles_p)};
}

// out[j] <- src[rr ? H-1-p : p][rc ? W-1-(q+j) : q+j], j = 0..3, for the pixels inside the plane (the others keep their value)
__device__ __forceinline__ void dihedral_quad_direct(const float* __restrict__ src, int H, int W, int p, int q, bool rr, bool rc, int vec, float (&out)[4]) {
    if (p >= H || q >= W) return;
    const float* row = src + (size_t)(rr ? H - 1 - p : p) * W;
    if (vec) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + (rc ? W - 4 - q : q));
        out[0] = rc ? v.w : v.x; out[1] = rc ? v.z : v.y; out[2] = rc ? v.y : v.z; out[3] = rc ? v.x : v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q + j < W) out[j] = row[rc ? W - 1 - (q + j) : q + j];
    }
}

// patch[q - q0][p - p0] <- src[rr ? N-1-q : q][rc ? N-1-p : p] for the tile's pixels inside the N x N plane (all 256 threads call it)
__device__ __forceinline__ void dihedral_stage_transposed(const float* __restrict__ src, int N, int p0, int q0, bool rr, bool rc, int vec, float* patch) {
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    dihedral_quad_direct(src, N, N, q0 + r, p0 + c4, rr, rc, vec, v);        // (the source tile is a non-transposing gather at (q0, p0))
    if (q0 + r < N) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + c4 + j < N) patch[r * DH_PITCH + c4 + j] = v[j];
    }
}

__device__ __forceinline__ void dihedral_quad_from_patch(const float* patch, float (&out)[4]) {
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = patch[(c4 + j) * DH_PITCH + r];     // (words outside the plane hold stale LDS: never stored to memory)
}

__device__ __forceinline__ void dihedral_store_quad(float* __restrict__ dst, int W, int p, int q, int vec, const float (&v)[4]) {
    float* o = dst + (size_t)p * W + q;
    if (vec) *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q + j < W) o[j] = v[j];
    }
}

// The fill: dst [n][C][Hv][Wv] <- view(images[(v0 + j) / G], code[(v0 + j) % G]) for the n virtual samples from v0 (image-major).
// grid (tiles of a view's plane * C, n); the code is uniform in the workgroup, so only workgroups of a transposing view touch LDS.
__global__ __launch_bounds__(256)
void dihedral_views_kernel(const float* __restrict__ images, float* __restrict__ dst, DihedralViews dv, int C, int H, int W, int v0, int vec) {
    __shared__ float patch[DH_PATCH];
    const unsigned v = (unsigned)v0 + blockIdx.y, G = (unsigned)dv.n;
    const unsigned img = v / G, code = dv.code[v - img * G];
    const bool t = code & 4, fy = code & 2, fx = code & 1;
    const DihedralTile tl = dihedral_tile(H, W);                              // (t: H == W, the view's plane has the image's shape)
    const size_t plane = (size_t)H * W;
    const float* src = images + ((size_t)img * C + tl.c) * plane;
    const int p = tl.p0 + (threadIdx.x >> 3), q = tl.q0 + (threadIdx.x & 7) * 4;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (t) {
        dihedral_stage_transposed(src, H, tl.p0, tl.q0, fx, fy, vec, patch);
        __syncthreads();
        dihedral_quad_from_patch(patch, x);
    } else {
        dihedral_quad_direct(src, H, W, p, q, fy, fx, vec, x);
    }
    if (p < H && q < W) dihedral_store_quad(dst + ((size_t)blockIdx.y * C + tl.c) * plane, W, p, q, vec, x);
}

static bool dihedral_views_ok(const DihedralViews& dv, int C, int H, int W, unsigned* grid_x) {
    if (dv.n < 1 || dv.n > DIHEDRAL_MAX_VIEWS || C < 1 || H < 1 || W < 1 || (unsigned long long)C * H * W >= (1ull << 32)) return false;
    for (int k = 0; k < dv.n; ++k)
        if (dv.code[k] > 7 || ((dv.code[k] & 4) && H != W)) return false;
    const unsigned long long blocks = (unsigned long long)((H + DH_T - 1) / DH_T) * ((W + DH_T - 1) / DH_T) * C;
    if (blocks > 2147483647ull) return false;
    *grid_x = (unsigned)blocks;
    return true;
}

static bool dihedral_transposes(const DihedralViews& dv) {
    for (int k = 0; k < dv.n; ++k)
        if (dv.code[k] & 4) return true;
    return false;
}

hipError_t dihedral_views_launch(const float* images, float* dst, const DihedralViews& dv, int C, int H, int W, int v0, int n, hipStream_t s) {
    unsigned gx = 0;
    if (!dihedral_views_ok(dv, C, H, W, &gx) || v0 < 0 || n < 1 || n > 65535 || !images || !dst) return hipErrorInvalidValue;
    const int vec = (W % 4 == 0 && ((size_t)H * W) % 4 == 0 && aligned16(images) && aligned16(dst)) ? 1 : 0;
    hipLaunchKernelGGL(dihedral_views_kernel, dim3(gx, n), dim3(256), 0, s, images, dst, dv, C, H, W, v0, vec);
    return hipGetLastError();
}

// The members of a thread's four pixels, turned back into the image's frame: x[k][j] = unview(views_out[b][k], code[k]) at the
// pixel, k = 0 .. G-1 in list order, in registers (the loop over the 8 possible views is unrolled: every index is a constant).
// TR (some view of the list transposes): every transposing view of the list gets an LDS patch of its own (at most four codes
// transpose), all are staged, ONE barrier, then every thread picks its pixels up.  !TR: no LDS, no barrier.
template <bool TR>
__device__ __forceinline__ void dihedral_gather_members(const float* __restrict__ views_b, const DihedralViews& dv, const DihedralTile& tl,
                                                        int C, int H, int W, int vec, float* patches, float (&x)[DIHEDRAL_MAX_VIEWS][4]) {
    const size_t plane = (size_t)H * W;
    const int p = tl.p0 + (threadIdx.x >> 3), q = tl.q0 + (threadIdx.x & 7) * 4;
    if constexpr (TR) {
        int slot = 0;
#pragma unroll
        for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k)
            if (k < dv.n && (dv.code[k] & 4)) {
                dihedral_stage_transposed(views_b + ((size_t)k * C + tl.c) * plane, H, tl.p0, tl.q0, dv.code[k] & 2, dv.code[k] & 1, vec,
                                          patches + slot * DH_PATCH);
                ++slot;
            }
        __syncthreads();
    }
    int slot = 0;
#pragma unroll
    for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[k][j] = 0.f;
        if (k < dv.n) {
            if (TR && (dv.code[k] & 4)) {
                dihedral_quad_from_patch(patches + slot * DH_PATCH, x[k]);
                ++slot;
            } else {
                dihedral_quad_direct(views_b + ((size_t)k * C + tl.c) * plane, H, W, p, q, dv.code[k] & 2, dv.code[k] & 1, vec, x[k]);
            }
        }
    }
}

// The final launch of mi_denoise_self_ensemble: views_out [B][G][C][Hv][Wv], the sampler outputs in each view's own frame, ->
// mean / unbiased std [B][C][H][W] over the G views turned back and, if asked for, those aligned members [B][G][C][H][W].
// THE ARITHMETIC IS FIXED (include/midd.h: mi_dihedral_reduce): the gather above, then exactly ensemble_reduce_kernel's sums over
// x_0 .. x_{G-1} in list order -- the result equals unview per view followed by mi_ensemble_reduce, bit for bit, with or without
// `samples`; the aligned members exist in memory only when the caller wants them.  grid (tiles of a plane * C, B)
template <bool TR>
__global__ __launch_bounds__(256)
void dihedral_reduce_kernel(const float* __restrict__ views_out, float* __restrict__ mean, float* __restrict__ stdv, float* __restrict__ samples,
                            DihedralViews dv, int C, int H, int W, int vec) {
    __shared__ float patches[TR ? 4 * DH_PATCH : 1];
    const DihedralTile tl = dihedral_tile(H, W);
    const size_t b = blockIdx.y, plane = (size_t)H * W, chw = (size_t)C * plane;
    const int G = dv.n;
    float x[DIHEDRAL_MAX_VIEWS][4];
    dihedral_gather_members<TR>(views_out + b * G * chw, dv, tl, C, H, W, vec, patches, x);
    const int p = tl.p0 + (threadIdx.x >> 3), q = tl.q0 + (threadIdx.x & 7) * 4;
    if (p >= H || q >= W) return;                            // (after the barrier)
    const size_t at = b * chw + (size_t)tl.c * plane;        // the pixel's [H][W] plane inside a [B][C][H][W] output
    double sum[4], m64[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] = 0.0;
#pragma unroll
    for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k)
        if (k < G) {
            if (samples) dihedral_store_quad(samples + (b * G + k) * chw + (size_t)tl.c * plane, W, p, q, vec, x[k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) sum[j] = add_rn64(sum[j], (double)x[k][j]);
        }
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { m64[j] = __ddiv_rn(sum[j], (double)G); out[j] = __double2float_rn(m64[j]); }
    if (mean) dihedral_store_quad(mean + at, W, p, q, vec, out);
    if (stdv) {
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
        dihedral_store_quad(stdv + at, W, p, q, vec, out);
    }
}

hipError_t dihedral_reduce_launch(const float* views_out, int B, const DihedralViews& dv, int C, int H, int W,
                                  float* mean, float* stdv, float* samples, hipStream_t s) {
    unsigned gx = 0;
    if (!dihedral_views_ok(dv, C, H, W, &gx) || B < 1 || B > 65535 || !views_out || (!mean && !stdv && !samples) || (stdv && dv.n < 2))
        return hipErrorInvalidValue;
    const int vec = (W % 4 == 0 && ((size_t)H * W) % 4 == 0 && aligned16(views_out) && aligned16(mean) && aligned16(stdv) && aligned16(samples)) ? 1 : 0;
    if (dihedral_transposes(dv))
        hipLaunchKernelGGL(dihedral_reduce_kernel<true>, dim3(gx, B), dim3(256), 0, s, views_out, mean, stdv, samples, dv, C, H, W, vec);
    else
        hipLaunchKernelGGL(dihedral_reduce_kernel<false>, dim3(gx, B), dim3(256), 0, s, views_out, mean, stdv, samples, dv, C, H, W, vec);
    return hipGetLastError();
}

// views_out [B][G][C][Hv][Wv] -> out [B][nq][C][H][W]: the gather above, then the sort and the interpolation of
// ensemble_quantiles_kernel over x_0 .. x_{G-1} (G <= 8: the one network of 8 keys): mi_ensemble_quantiles of the aligned members,
// bit for bit, which never exist in memory.  Keys and members at constant register indices only: no scratch.  grid as above
template <bool TR>
__global__ __launch_bounds__(256)
void dihedral_quantiles_kernel(const float* __restrict__ views_out, float* __restrict__ out, DihedralViews dv, QuantileLevels ql,
                               int C, int H, int W, int vec) {
    __shared__ float patches[TR ? 4 * DH_PATCH : 1];
    const DihedralTile tl = dihedral_tile(H, W);
    const size_t b = blockIdx.y, plane = (size_t)H * W, chw = (size_t)C * plane;
    const int G = dv.n;
    float x[DIHEDRAL_MAX_VIEWS][4];
    dihedral_gather_members<TR>(views_out + b * G * chw, dv, tl, C, H, W, vec, patches, x);
    const int p = tl.p0 + (threadIdx.x >> 3), q = tl.q0 + (threadIdx.x & 7) * 4;
    if (p >= H || q >= W) return;                            // (after the barrier)
    uint32_t key[4][DIHEDRAL_MAX_VIEWS];
    bool has_nan[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        has_nan[j] = false;
#pragma unroll
        for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k) {
            const uint32_t bits = __float_as_uint(x[k][j]);
            key[j][k] = (k < G) ? order_key(bits) : ORDER_KEY_PAD;
            has_nan[j] = has_nan[j] || (k < G && is_nan_bits(bits));
        }
        sort_keys<DIHEDRAL_MAX_VIEWS>(key[j]);
    }
    float* dst = out + b * (size_t)ql.nq * chw + (size_t)tl.c * plane;
    for (int i = 0; i < ql.nq; ++i) {
        const QuantilePos pos = quantile_pos(ql.q[i], G);
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = quantile_of_sorted<DIHEDRAL_MAX_VIEWS>(key[j], pos, G, has_nan[j]);
        dihedral_store_quad(dst + (size_t)i * chw, W, p, q, vec, r);
    }
}

hipError_t dihedral_quantiles_launch(const float* views_out, int B, const DihedralViews& dv, int C, int H, int W,
                                     const QuantileLevels& ql, float* out, hipStream_t s) {
    unsigned gx = 0;
    if (!dihedral_views_ok(dv, C, H, W, &gx) || B < 1 || B > 65535 || !views_out || !out || !quantile_levels_ok(ql)) return hipErrorInvalidValue;
    const int vec = (W % 4 == 0 && ((size_t)H * W) % 4 == 0 && aligned16(views_out) && aligned16(out)) ? 1 : 0;
    if (dihedral_transposes(dv))
        hipLaunchKernelGGL(dihedral_quantiles_kernel<true>, dim3(gx, B), dim3(256), 0, s, views_out, out, dv, ql, C, H, W, vec);
    else
        hipLaunchKernelGGL(dihedral_quantiles_kernel<false>, dim3(gx, B), dim3(256), 0, s, views_out, out, dv, ql, C, H, W, vec);
    return hipGetLastError();
}

}  // namespace midd
