// The resampling kernels of the UNet and the layout helpers.
//
//   resize_bilinear  : F.interpolate(mode='bilinear', align_corners=False) (DDIMModel.py:242)
//   conv_transpose   : ConvTranspose2d(C,C,4,2,1) (DDIMModel.py:211) for topologies where the
//                      planner cannot fold it into a 3x3 (never on the default networks)
//   nhwc_to_nchw, fill_i32 : an activation tensor as NCHW; a few integers into device memory
// The resize is HBM-bound and judged against the HBM roofline.
#include "midd_internal.h"
#include "pointwise_common.h"

namespace midd {

// ------------------------------------------------------------------------------ bilinear resize (NHWC; the channel-blocked variant follows)
// Same index/weight arithmetic as ATen's upsample_bilinear2d with align_corners=False:
//   src = max(0, scale*(dst+0.5)-0.5), scale = in/out;  i0 = floor(src), i1 = i0 + (i0 < in-1), l1 = src - i0.
// grid (rows, B); also leaves the GroupNorm totals of its output (pointwise_publish)
__global__ __launch_bounds__(256)
void resize_bilinear_kernel(const float* __restrict__ src, float* __restrict__ dst, stat_word* __restrict__ tot, int rep, int bs,
                            int H, int W, int C, int OH, int OW, float sy, float sx, int rows) {
    extern __shared__ float rs_lds[];             // statistics scratch
    const int CQ = C >> 2;
    const int ppi = 256 / CQ;
    const int tid = threadIdx.x;
    const int pl = tid / CQ, cq = tid - pl * CQ;
    const bool active = pl < ppi;
    const int b = blockIdx.y, row = blockIdx.x;
    const int OHW = OH * OW;
    const int per = (OHW + rows - 1) / rows;
    const int p0 = row * per, p1 = min(OHW, p0 + per);
    float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const float* base = src + (size_t)b * H * W * C + cq * 4;
        for (int p = p0 + pl; p < p1; p += ppi) {
            const int oy = p / OW, ox = p - oy * OW;
            float fy = sy * ((float)oy + 0.5f) - 0.5f; if (fy < 0.f) fy = 0.f;
            float fx = sx * ((float)ox + 0.5f) - 0.5f; if (fx < 0.f) fx = 0.f;
            const int y0 = (int)fy, x0 = (int)fx;
            const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
            const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
            const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
            const f32x4 v00 = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * W + x0) * C);
            const f32x4 v01 = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * W + x1) * C);
            const f32x4 v10 = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * W + x0) * C);
            const f32x4 v11 = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * W + x1) * C);
            const f32x4 r = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
            *reinterpret_cast<f32x4*>(dst + ((size_t)b * OHW + p) * C + cq * 4) = r;
#pragma unroll
            for (int e = 0; e < 4; ++e) { ssum[e] += r[e]; ssq[e] += r[e] * r[e]; }
        }
    }
    if (tot == nullptr) return;
    stat_word* const acc_lds = reinterpret_cast<stat_word*>(rs_lds + 2 * (size_t)C * ppi);       // C % 4 == 0: 8-byte aligned
    pointwise_publish<4>(ssum, ssq, active, pl, ppi, cq, C, rs_lds, acc_lds, tot, b, bs, rep, row % rep, tid);
}

// Channel-blocked tensors [B][C/16][H][W][16] (midd_internal.h): grid (rows, B, C/16), thread = (pixel lane 0..63, quad 0..3 of
// the block) -- a wave reads and writes whole contiguous runs of 16 pixels x 64 bytes.  Same arithmetic and statistics as above.
__global__ __launch_bounds__(256)
void resize_bilinear_blocked_kernel(const float* __restrict__ src, float* __restrict__ dst, stat_word* __restrict__ tot, int rep, int bs,
                                    int H, int W, int C, int OH, int OW, float sy, float sx, int rows) {
    __shared__ float rs_scratch[2 * 16 * 64];
    __shared__ stat_word rs_acc[(16 + 2) * STAT_WORDS];
    const int tid = threadIdx.x;
    const int pl = tid >> 2, q = tid & 3;
    const int b = blockIdx.y, row = blockIdx.x, blk = blockIdx.z;
    const int OHW = OH * OW;
    const int per = (OHW + rows - 1) / rows;
    const int p0 = row * per, p1 = min(OHW, p0 + per);
    float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
    const float* base = src + (((size_t)b * (C >> 4) + blk) * (size_t)(H * W)) * 16 + q * 4;
    float* const obase = dst + (((size_t)b * (C >> 4) + blk) * (size_t)OHW) * 16 + q * 4;
    for (int p = p0 + pl; p < p1; p += 64) {
        const int oy = p / OW, ox = p - oy * OW;
        float fy = sy * ((float)oy + 0.5f) - 0.5f; if (fy < 0.f) fy = 0.f;
        float fx = sx * ((float)ox + 0.5f) - 0.5f; if (fx < 0.f) fx = 0.f;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
        const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
        const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
        const f32x4 v00 = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * W + x0) * 16);
        const f32x4 v01 = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * W + x1) * 16);
        const f32x4 v10 = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * W + x0) * 16);
        const f32x4 v11 = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * W + x1) * 16);
        const f32x4 r = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
        *reinterpret_cast<f32x4*>(obase + (size_t)p * 16) = r;
#pragma unroll
        for (int e = 0; e < 4; ++e) { ssum[e] += r[e]; ssq[e] += r[e] * r[e]; }
    }
    if (tot == nullptr) return;
    pointwise_publish<4>(ssum, ssq, true, pl, 64, q, C, rs_scratch, rs_acc, tot, b, bs, rep, row % rep, tid, 256, blk * 16, 16);
}

hipError_t resize_bilinear_launch(const float* src, float* dst, stat_word* tot, int rep, int bs, int B, int H, int W, int C, int OH, int OW, int blocked, hipStream_t s) {
    if (blocked) {
        if (C % 16) return hipErrorInvalidValue;
        const int rows_b = pointwise_rows(OH * OW, 64);
        hipLaunchKernelGGL(resize_bilinear_blocked_kernel, dim3(rows_b, B, C / 16), dim3(256), 0, s,
                           src, dst, tot, rep, bs, H, W, C, OH, OW, (float)H / (float)OH, (float)W / (float)OW, rows_b);
        return hipGetLastError();
    }
    if (C % 4 || C / 4 > 256) return hipErrorInvalidValue;
    const int ppi = 256 / (C / 4);
    const int rows = pointwise_rows(OH * OW, ppi);
    const size_t lds = (size_t)2 * C * ppi * sizeof(float) + (size_t)(C + 2) * STAT_WORDS * sizeof(stat_word);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3(rows, B), dim3(256), lds, s,
                       src, dst, tot, rep, bs, H, W, C, OH, OW, (float)H / (float)OH, (float)W / (float)OW, rows);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ ConvTranspose2d(4,2,1) direct
// out[oy][ox][co] = bias[co] + sum_{ky,kx,ci} in[(oy+1-ky)/2][(ox+1-kx)/2][ci] * w[ky][kx][ci][co]
// over taps with (oy+1-ky), (ox+1-kx) even and in range.  Thread = (output pixel, 4 couts).
__global__ __launch_bounds__(256)
void conv_transpose_kernel(const float* __restrict__ src, const float* __restrict__ w, const float* __restrict__ bias,
                           float* __restrict__ dst, int B, int H, int W, int Cin, int Cout, int blocked) {
    const int OH = 2 * H, OW = 2 * W, CQ = Cout >> 2;
    const long total = (long)B * OH * OW * CQ;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int cq = (int)(gid % CQ);
    const long pix = gid / CQ;
    const int ox = (int)(pix % OW);
    const int oy = (int)((pix / OW) % OH);
    const int b = (int)(pix / ((long)OW * OH));
    f32x4 acc = *reinterpret_cast<const f32x4*>(bias + cq * 4);
    for (int ky = 0; ky < 4; ++ky) {
        const int ny = oy + 1 - ky;
        if (ny < 0 || (ny & 1) || (ny >> 1) >= H) continue;
        for (int kx = 0; kx < 4; ++kx) {
            const int nx = ox + 1 - kx;
            if (nx < 0 || (nx & 1) || (nx >> 1) >= W) continue;
            const int ipix = (ny >> 1) * W + (nx >> 1);
            const float* wp = w + ((size_t)(ky * 4 + kx) * Cin) * Cout + cq * 4;
            for (int ci = 0; ci < Cin; ++ci)
                acc += src[act_index(blocked, b, Cin, H * W, ipix, ci)] * *reinterpret_cast<const f32x4*>(wp + (size_t)ci * Cout);
        }
    }
    *reinterpret_cast<f32x4*>(dst + act_index(blocked, b, Cout, OH * OW, oy * OW + ox, cq * 4)) = acc;
}

hipError_t conv_transpose_launch(const float* src, const float* w, const float* bias, float* dst,
                                 int B, int H, int W, int Cin, int Cout, int blocked, hipStream_t s) {
    if (Cout % 4) return hipErrorInvalidValue;
    const long total = (long)B * 4 * H * W * (Cout / 4);
    hipLaunchKernelGGL(conv_transpose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       src, w, bias, dst, B, H, W, Cin, Cout, blocked);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ helpers
__global__ void nhwc_to_nchw_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int H, int W, int C, int blocked) {
    const long total = (long)B * H * W * C;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int c = (int)(gid % C);
    const long pix = gid / C;
    const long hw = pix % ((long)H * W);
    const int b = (int)(pix / ((long)H * W));
    dst[((size_t)b * C + c) * H * W + hw] = src[act_index(blocked, b, C, H * W, (int)hw, c)];
}

hipError_t nhwc_to_nchw_launch(const float* src, float* dst, int B, int H, int W, int C, int blocked, hipStream_t s) {
    const long total = (long)B * H * W * C;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, B, H, W, C, blocked);
    return hipGetLastError();
}

struct I32x32 { int v[32]; };
__global__ void fill_i32_kernel(int* dst, I32x32 vals, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
}

hipError_t fill_i32_launch(int* dst, const int* host_vals, int n, hipStream_t s) {
    for (int i = 0; i < n; i += 32) {
        I32x32 v;
        const int m = (n - i < 32) ? n - i : 32;
        for (int j = 0; j < 32; ++j) v.v[j] = (j < m) ? host_vals[i + j] : 0;
        hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(32), 0, s, dst + i, v, m);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace midd
