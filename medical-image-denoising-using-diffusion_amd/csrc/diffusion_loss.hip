// The training objective as an evaluation (DDIMModel.py:259-266, :351-375; cddpmModels.py:367-374): the forward noising
// x_t = a * clean + s * eps and the per-sample denoising loss -- the MSE of the predicted noise plus the L1 distance between the Sobel
// edge magnitudes of the predicted clean image and of the clean image.  The specification is in include/midd.h (THE FORWARD NOISE,
// THE NOISING, THE DENOISING LOSS); tests/denoising_loss_reference.py restates it in numpy.
//   noise_images_kernel<seeded>   x_t (and, seeded, eps) of a batch: 16-byte body with a scalar head and tail per sample, all scalar
//                                 when the tensors of the call do not share one misalignment
//   loss_terms_kernel<seeded>     a workgroup owns a 32 x 32 patch of one channel of one sample: it forms p and clean of the 34 x 34
//                                 halo patch once in LDS (zero outside the image), applies the two stencils, and leaves the patch's two
//                                 sums; seeded, z and x_t are formed again instead of read.  Both forms run loss_pixel, so they agree
//                                 bit for bit
//   loss_final_kernel             one thread per sample adds its partial sums in the specified order -> (mse, edge, loss)
// Contraction is off for the whole unit and the arithmetic is written with the plain operators (hipcc's __fmul_rn / __fadd_rn are
// those operators compiled where contraction is allowed: -ffp-contract=fast fuses them): the only fused multiply-adds left in the ISA
// are inside the correctly rounded division and square root and the library's logf / cospif.  No floating-point atomics.
#include "midd_internal.h"
#include "step_noise_common.h"

#pragma clang fp contract(off)

namespace midd {

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_HALO = LOSS_PATCH + 2;       // 34: the patch with its one-pixel border
// LDS pitch of the halo patch.  The stencil phase reads a row of 32 consecutive columns per 32-lane half (ds_read_b32 banks are
// (address / 4) % 32 per half): 32 distinct banks at every one of the nine taps whatever the pitch.  The fill phase writes
// consecutive words only at pitch == LOSS_HALO, so that is the pitch.
constexpr int LOSS_PITCH = LOSS_HALO;
static_assert(LOSS_PATCH == 32 && LOSS_THREADS == 256, "loss_terms_kernel: 8 rows of 32 threads, four pixels a thread");

// torch.clamp: a NaN stays a NaN (fminf / fmaxf would drop it)
__device__ __forceinline__ float clamp_keep_nan(float v, float lo, float hi) { return v < lo ? lo : (v > hi ? hi : v); }

// THE NOISING: two products and one sum, each rounded once
__device__ __forceinline__ float noised(float a, float s, float clean, float eps) {
    const float pa = a * clean, ps = s * eps;
    return pa + ps;
}

template <bool SEEDED>
__global__ __launch_bounds__(LOSS_THREADS)
void noise_images_kernel(const float* __restrict__ clean, const float* __restrict__ eps, float* __restrict__ x_t,
                         float* __restrict__ eps_out, LossRecs recs, int b0, unsigned long long chw, unsigned long long seed) {
    const LossRec rec = recs.v[blockIdx.y];
    const size_t base = (size_t)(b0 + (int)blockIdx.y) * chw;
    const float* c = clean + base;
    float* xo = x_t + base;
    const float* ei = SEEDED ? nullptr : eps + base;
    float* eo = (SEEDED && eps_out) ? eps_out + base : nullptr;
    // elements before the first 16-byte boundary of this sample's row; the 16-byte body needs every tensor to share it
    const unsigned mis = (unsigned)((reinterpret_cast<uintptr_t>(c) >> 2) & 3);
    bool same = ((reinterpret_cast<uintptr_t>(xo) >> 2) & 3) == mis;
    if (SEEDED) same = same && (!eo || ((reinterpret_cast<uintptr_t>(eo) >> 2) & 3) == mis);
    else same = same && ((reinterpret_cast<uintptr_t>(ei) >> 2) & 3) == mis;
    unsigned long long head = same ? (unsigned long long)((4u - mis) & 3u) : chw;
    if (head > chw) head = chw;
    const unsigned long long nvec = (chw - head) >> 2, tail = head + 4 * nvec;
    const unsigned long long tid = (unsigned long long)blockIdx.x * LOSS_THREADS + threadIdx.x, stride = (unsigned long long)gridDim.x * LOSS_THREADS;
    for (unsigned long long v = tid; v < nvec; v += stride) {
        const unsigned long long i = head + 4 * v;
        const float4 cv = *reinterpret_cast<const float4*>(c + i);
        float4 n;
        if (SEEDED) {
            n.x = forward_noise_value(seed, rec.sample, rec.draw, (uint32_t)i);
            n.y = forward_noise_value(seed, rec.sample, rec.draw, (uint32_t)(i + 1));
            n.z = forward_noise_value(seed, rec.sample, rec.draw, (uint32_t)(i + 2));
            n.w = forward_noise_value(seed, rec.sample, rec.draw, (uint32_t)(i + 3));
            if (eo) *reinterpret_cast<float4*>(eo + i) = n;
        } else {
            n = *reinterpret_cast<const float4*>(ei + i);
        }
        float4 o;
        o.x = noised(rec.a, rec.s, cv.x, n.x); o.y = noised(rec.a, rec.s, cv.y, n.y);
        o.z = noised(rec.a, rec.s, cv.z, n.z); o.w = noised(rec.a, rec.s, cv.w, n.w);
        *reinterpret_cast<float4*>(xo + i) = o;
    }
    const unsigned long long nscalar = head + (chw - tail);
    for (unsigned long long j = tid; j < nscalar; j += stride) {
        const unsigned long long i = j < head ? j : tail + (j - head);
        float n;
        if (SEEDED) {
            n = forward_noise_value(seed, rec.sample, rec.draw, (uint32_t)i);
            if (eo) eo[i] = n;
        } else {
            n = ei[i];
        }
        xo[i] = noised(rec.a, rec.s, c[i], n);
    }
}

// One pixel of THE DENOISING LOSS: q = (e - eps)^2 and the predicted clean image p, from the pixel's clean value, predicted noise and
// -- read (explicit) or formed again (seeded) -- x_t and eps.  The one function behind both instantiations of the kernel.
struct LossPixel { float q, p; };
__device__ __forceinline__ LossPixel loss_pixel(float a, float s, float x_t, float eps, float eps_pred, int clamp_eps) {
    const float e = clamp_eps ? clamp_keep_nan(eps_pred, -5.0f, 5.0f) : eps_pred;
    const float d = e - eps;
    LossPixel r;
    r.q = d * d;
    const float se = s * e;
    r.p = clamp_keep_nan((x_t - se) / a, 0.0f, 1.0f);
    return r;
}

// Sobel magnitude at the pixel whose 3 x 3 neighbourhood starts at u (LDS, pitch LOSS_PITCH): the six non-zero taps of each kernel in
// row-major order, every sum rounded on its own (the products by 1 and 2 are exact)
__device__ __forceinline__ float sobel_magnitude(const float* u) {
    const float u00 = u[0], u01 = u[1], u02 = u[2], u10 = u[LOSS_PITCH], u12 = u[LOSS_PITCH + 2];
    const float u20 = u[2 * LOSS_PITCH], u21 = u[2 * LOSS_PITCH + 1], u22 = u[2 * LOSS_PITCH + 2];
    float ex = -u00;
    ex = ex + u02;
    ex = ex - 2.0f * u10;
    ex = ex + 2.0f * u12;
    ex = ex - u20;
    ex = ex + u22;
    float ey = -u00;
    ey = ey - 2.0f * u01;
    ey = ey - u02;
    ey = ey + u20;
    ey = ey + 2.0f * u21;
    ey = ey + u22;
    const float xx = ex * ex, yy = ey * ey;
    return sqrtf((xx + yy) + 1e-8f);      // correctly rounded (hipcc's __fsqrt_rn is the 1-ulp native instruction)
}

// grid (tiles_y * tiles_x, C, samples of this launch)
template <bool SEEDED>
__global__ __launch_bounds__(LOSS_THREADS)
void loss_terms_kernel(const float* __restrict__ clean, const float* __restrict__ x_t, const float* __restrict__ eps,
                       const float* __restrict__ eps_pred, LossRecs recs, int b0, int C, int H, int W, int tiles_x,
                       unsigned long long seed, int clamp_eps,
                       float* __restrict__ map_q, float* __restrict__ map_g, float* __restrict__ map_p, double* __restrict__ part) {
    __shared__ float sp[LOSS_HALO * LOSS_PITCH], sc[LOSS_HALO * LOSS_PITCH], sq[LOSS_PATCH * LOSS_PATCH];
    __shared__ double red[LOSS_THREADS][2];
    const LossRec rec = recs.v[blockIdx.z];
    const int b = b0 + (int)blockIdx.z, c = blockIdx.y, tile = blockIdx.x;
    const int y0 = (tile / tiles_x) * LOSS_PATCH, x0 = (tile % tiles_x) * LOSS_PATCH;
    const size_t plane = ((size_t)b * C + c) * ((size_t)H * W);               // offset of this sample's channel in the tensors
    const uint32_t elem0 = (uint32_t)((unsigned long long)c * H * W);          // its first element index inside the sample (C*H*W < 2^32)
    const int tid = threadIdx.x;

    // the halo patch, every pixel once: p and clean (zero outside the image), q of the pixels the patch owns
    for (int i = tid; i < LOSS_HALO * LOSS_HALO; i += LOSS_THREADS) {
        const int hy = i / LOSS_HALO, hx = i % LOSS_HALO;
        const int y = y0 + hy - 1, x = x0 + hx - 1;
        float pv = 0.0f, cv = 0.0f, qv = 0.0f;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t in_plane = (size_t)y * W + x;
            cv = clean[plane + in_plane];
            float n, xt;
            if (SEEDED) {
                n = forward_noise_value(seed, rec.sample, rec.draw, elem0 + (uint32_t)in_plane);
                xt = noised(rec.a, rec.s, cv, n);
            } else {
                n = eps[plane + in_plane];
                xt = x_t[plane + in_plane];
            }
            const LossPixel r = loss_pixel(rec.a, rec.s, xt, n, eps_pred[plane + in_plane], clamp_eps);
            pv = r.p; qv = r.q;
        }
        sp[hy * LOSS_PITCH + hx] = pv;
        sc[hy * LOSS_PITCH + hx] = cv;
        if (hy >= 1 && hy <= LOSS_PATCH && hx >= 1 && hx <= LOSS_PATCH) sq[(hy - 1) * LOSS_PATCH + hx - 1] = qv;
    }
    __syncthreads();

    // thread j owns column j % 32 of rows j / 32 + 8 k, k = 0 .. 3, added in that order
    const int lx = tid & (LOSS_PATCH - 1), ly0 = tid / LOSS_PATCH;
    double sum_q = 0.0, sum_g = 0.0;
#pragma unroll
    for (int k = 0; k < LOSS_PATCH * LOSS_PATCH / LOSS_THREADS; ++k) {
        const int ly = ly0 + k * (LOSS_THREADS / LOSS_PATCH);
        const int y = y0 + ly, x = x0 + lx;
        if (y < H && x < W) {
            const float g = fabsf(sobel_magnitude(sp + ly * LOSS_PITCH + lx) - sobel_magnitude(sc + ly * LOSS_PITCH + lx));
            const float q = sq[ly * LOSS_PATCH + lx];
            sum_q = sum_q + (double)q;
            sum_g = sum_g + (double)g;
            const size_t at = plane + (size_t)y * W + x;
            if (map_q) map_q[at] = q;
            if (map_g) map_g[at] = g;
            if (map_p) map_p[at] = sp[(ly + 1) * LOSS_PITCH + lx + 1];
        }
    }
    red[tid][0] = sum_q; red[tid][1] = sum_g;
    __syncthreads();
    for (int off = LOSS_THREADS / 2; off > 0; off >>= 1) {      // fixed tree: v[j] += v[j + off]
        if (tid < off) {
            red[tid][0] = red[tid][0] + red[tid + off][0];
            red[tid][1] = red[tid][1] + red[tid + off][1];
        }
        __syncthreads();
    }
    if (tid == 0) {
        double* o = part + (((size_t)b * C + c) * gridDim.x + tile) * 2;
        o[0] = red[0][0]; o[1] = red[0][1];
    }
}

// one thread per sample: its partial sums in (channel, tile row, tile column) order
__global__ void loss_final_kernel(const double* __restrict__ part, int B, int per_sample, double count, double edge_weight, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double* p = part + (size_t)b * per_sample * 2;
    double sq = 0.0, sg = 0.0;
    for (int i = 0; i < per_sample; ++i) { sq = sq + p[2 * i]; sg = sg + p[2 * i + 1]; }
    const double mse = sq / count, edge = sg / count;
    out[3 * b] = mse;
    out[3 * b + 1] = edge;
    const double weighted = edge_weight * edge;
    out[3 * b + 2] = mse + weighted;
}

// ---------------------------------------------------------------------------------------------------------------- launches
hipError_t noise_images_launch(const float* clean, const float* eps, float* x_t, float* eps_out, const LossRec* recs, int B,
                               unsigned long long chw, int seeded, unsigned long long seed, hipStream_t s) {
    if (B < 1 || chw < 1 || chw > 0xffffffffull || (seeded != 0) == (eps != nullptr) || (!seeded && eps_out)) return hipErrorInvalidValue;
    const unsigned long long groups = (chw + 4 * LOSS_THREADS - 1) / (4 * LOSS_THREADS);
    const unsigned gx = (unsigned)(groups < 4096 ? groups : 4096);      // grid-stride beyond that
    for (int b0 = 0; b0 < B; b0 += LOSS_RECS_PER_LAUNCH) {
        const int n = B - b0 < LOSS_RECS_PER_LAUNCH ? B - b0 : LOSS_RECS_PER_LAUNCH;
        LossRecs r{};
        for (int j = 0; j < n; ++j) r.v[j] = recs[b0 + j];
        if (seeded) hipLaunchKernelGGL(noise_images_kernel<true>, dim3(gx, n), dim3(LOSS_THREADS), 0, s, clean, eps, x_t, eps_out, r, b0, chw, seed);
        else hipLaunchKernelGGL(noise_images_kernel<false>, dim3(gx, n), dim3(LOSS_THREADS), 0, s, clean, eps, x_t, eps_out, r, b0, chw, seed);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

size_t loss_partials_bytes(int B, int C, int H, int W) { return (size_t)B * C * loss_tiles(H, W) * 2 * sizeof(double); }

hipError_t loss_terms_launch(const float* clean, const float* x_t, const float* eps, const float* eps_pred, const LossRec* recs,
                             int B, int C, int H, int W, int seeded, unsigned long long seed, int clamp_eps,
                             double edge_weight, double* out, float* maps, double* part, hipStream_t s) {
    const unsigned long long chw = (unsigned long long)C * H * W;
    if (B < 1 || C < 1 || C > 65535 || H < 1 || W < 1 || chw > 0xffffffffull) return hipErrorInvalidValue;
    if (seeded ? (x_t || eps) : (!x_t || !eps)) return hipErrorInvalidValue;
    const int tiles_x = (W + LOSS_PATCH - 1) / LOSS_PATCH, tiles = loss_tiles(H, W);
    float* mq = maps;
    float* mg = maps ? maps + (size_t)B * chw : nullptr;
    float* mp = maps ? maps + 2 * (size_t)B * chw : nullptr;
    for (int b0 = 0; b0 < B; b0 += LOSS_RECS_PER_LAUNCH) {
        const int n = B - b0 < LOSS_RECS_PER_LAUNCH ? B - b0 : LOSS_RECS_PER_LAUNCH;
        LossRecs r{};
        for (int j = 0; j < n; ++j) r.v[j] = recs[b0 + j];
        const dim3 grid(tiles, C, n);
        if (seeded) hipLaunchKernelGGL(loss_terms_kernel<true>, grid, dim3(LOSS_THREADS), 0, s, clean, x_t, eps, eps_pred, r, b0, C, H, W, tiles_x,
                                       seed, clamp_eps, mq, mg, mp, part);
        else hipLaunchKernelGGL(loss_terms_kernel<false>, grid, dim3(LOSS_THREADS), 0, s, clean, x_t, eps, eps_pred, r, b0, C, H, W, tiles_x,
                                seed, clamp_eps, mq, mg, mp, part);
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(loss_final_kernel, dim3((B + 63) / 64), dim3(64), 0, s, part, B, C * tiles, (double)chw, edge_weight, out);
    return hipGetLastError();
}

}  // namespace midd
