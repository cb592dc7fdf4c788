// Pre/post-processing either side of the sampler, on the device:
//   * Pillow's 8-bit bicubic resample (`transforms.Resize(..., BICUBIC)` / `Image.resize(size, Image.BICUBIC)` on an
//     'L' image: Backend/run.py:146,198; cddpmModels.py:488,502), bit for bit: separable, horizontal pass first,
//     coefficients normalised in double precision and rounded to 22-bit fixed point, int32 accumulation from 1 << 21,
//     arithmetic shift, clip, uint8 between the passes.  The coefficient tables are computed ON THE DEVICE in fp64
//     with FMA contraction off (same IEEE operations as Pillow's C), so the whole call is asynchronous.
//   * ToTensor (uint8 / 255 in fp32) and its inverse `(clamp(x, 0, 1) * 255).astype(uint8)` (run.py:107,145).
//   * PSNR / SSIM of `compute_metrics` (DDIMModel.py:290-300; skimage defaults: 7x7 uniform window, K1 = .01,
//     K2 = .03, sample covariance, mean over the interior), fp64, fixed summation order.
// Checker: oracle/resize_oracle.py (pinned against Pillow itself on the CPU); tests/test_gpu_prepost.py.
#include "../../include/midd.h"
#include "midd_internal.h"
#include <cstdint>
#include <type_traits>

namespace midd {

constexpr int PRECISION_BITS = 32 - 8 - 2;

__device__ __forceinline__ double bicubic_w(double x) {
#pragma clang fp contract(off)
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1.0;
    if (x < 2.0) return (((x - 5.0) * x + 8.0) * x - 4.0) * a;
    return 0.0;
}

// one thread per output index: bounds[xx] = (first tap, taps), kk[xx][0..ksize) fixed-point coefficients
__global__ void resize_coeffs_kernel(int in_size, int out_size, int ksize, int* __restrict__ bounds, int* __restrict__ kk) {
#pragma clang fp contract(off)
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    if (xx >= out_size) return;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bicubic_w((x + xmin - center + 0.5) * ss);
    int* k = kk + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
        int q = 0;
        if (x < xmax) {
            double w = bicubic_w((x + xmin - center + 0.5) * ss);
            if (ww != 0.0) w /= ww;
            q = (w < 0.0) ? (int)(-0.5 + w * (double)(1 << PRECISION_BITS)) : (int)(0.5 + w * (double)(1 << PRECISION_BITS));
        }
        k[x] = q;
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
}

__device__ __forceinline__ uint8_t clip8(int acc) {
    const int v = acc >> PRECISION_BITS;                 // arithmetic shift, as Pillow's lookup of (in >> PRECISION_BITS)
    return (uint8_t)(v < 0 ? 0 : (v > 255 ? 255 : v));
}

// rows = n * h rows of sw pixels -> rows of dw pixels
__global__ void resample_h_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, long rows, int sw, int dw,
                                     const int* __restrict__ bounds, const int* __restrict__ kk, int ksize) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * dw) return;
    const long row = idx / dw;
    const int xx = (int)(idx - row * dw);
    const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
    const int* k = kk + (size_t)xx * ksize;
    const uint8_t* s = src + row * sw + xmin;
    int acc = 1 << (PRECISION_BITS - 1);
    for (int x = 0; x < xmax; ++x) acc += (int)s[x] * k[x];
    dst[idx] = clip8(acc);
}

// n images of sh x w -> dh x w
__global__ void resample_v_u8_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int n, int sh, int dh, int w,
                                     const int* __restrict__ bounds, const int* __restrict__ kk, int ksize) {
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * dh * w) return;
    const int x = (int)(idx % w);
    const long t = idx / w;
    const int yy = (int)(t % dh);
    const int img = (int)(t / dh);
    const int ymin = bounds[2 * yy], ymax = bounds[2 * yy + 1];
    const int* k = kk + (size_t)yy * ksize;
    const uint8_t* s = src + ((size_t)img * sh + ymin) * w + x;
    int acc = 1 << (PRECISION_BITS - 1);
    for (int y = 0; y < ymax; ++y) acc += (int)s[(size_t)y * w] * k[y];
    dst[idx] = clip8(acc);
}

__global__ void u8_to_unit_kernel(const uint8_t* __restrict__ src, float* __restrict__ dst, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = __fdiv_rn((float)src[i], 255.0f);
}

__global__ void unit_to_u8_kernel(const float* __restrict__ src, uint8_t* __restrict__ dst, size_t count) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    float v = src[i];
    v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    dst[i] = (uint8_t)__fmul_rn(v, 255.0f);             // truncation, as ndarray.astype('uint8') on [0, 255]
}

static int resize_ksize(int in_size, int out_size) {
    const double scale = (double)in_size / (double)out_size;
    const double support = 2.0 * (scale < 1.0 ? 1.0 : scale);
    return (int)ceil(support) * 2 + 1;
}

// workspace: [h bounds 2*dw][h kk dw*ksize_h][v bounds 2*dh][v kk dh*ksize_v] ints, then the n*sh*dw intermediate
size_t resize_workspace_bytes(int n, int sw, int sh, int dw, int dh) {
    const size_t ints = 2 * (size_t)dw + (size_t)dw * resize_ksize(sw, dw) + 2 * (size_t)dh + (size_t)dh * resize_ksize(sh, dh);
    return ((ints * sizeof(int) + 255) & ~(size_t)255) + (size_t)n * sh * dw + 256;
}

hipError_t resize_bicubic_u8_launch(const uint8_t* src, int n, int sw, int sh, uint8_t* dst, int dw, int dh, void* ws, hipStream_t s) {
    if (n < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1) return hipErrorInvalidValue;
    const int kh = resize_ksize(sw, dw), kv = resize_ksize(sh, dh);
    int* hb = reinterpret_cast<int*>(ws);
    int* hk = hb + 2 * (size_t)dw;
    int* vb = hk + (size_t)dw * kh;
    int* vk = vb + 2 * (size_t)dh;
    const size_t ints = 2 * (size_t)dw + (size_t)dw * kh + 2 * (size_t)dh + (size_t)dh * kv;
    uint8_t* mid = reinterpret_cast<uint8_t*>(ws) + ((ints * sizeof(int) + 255) & ~(size_t)255);
    const uint8_t* cur = src;
    int cw = sw;
    const bool need_h = dw != sw, need_v = dh != sh;
    if (!need_h && !need_v) return hipMemcpyAsync(dst, src, (size_t)n * sh * sw, hipMemcpyDeviceToDevice, s);
    if (need_h) {
        hipLaunchKernelGGL(resize_coeffs_kernel, dim3((dw + 127) / 128), dim3(128), 0, s, sw, dw, kh, hb, hk);
        uint8_t* out = need_v ? mid : dst;
        const long total = (long)n * sh * dw;
        hipLaunchKernelGGL(resample_h_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cur, out, (long)n * sh, sw, dw, hb, hk, kh);
        cur = out; cw = dw;
    }
    if (need_v) {
        hipLaunchKernelGGL(resize_coeffs_kernel, dim3((dh + 127) / 128), dim3(128), 0, s, sh, dh, kv, vb, vk);
        const long total = (long)n * dh * cw;
        hipLaunchKernelGGL(resample_v_u8_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, cur, dst, n, sh, dh, cw, vb, vk, kv);
    }
    return hipGetLastError();
}

hipError_t u8_to_unit_launch(const uint8_t* src, float* dst, size_t count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(u8_to_unit_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, src, dst, count);
    return hipGetLastError();
}

hipError_t unit_to_u8_launch(const float* src, uint8_t* dst, size_t count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL(unit_to_u8_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, src, dst, count);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ high bit depth (include/midd.h: THE FLOAT RESIZE)
// Pillow's 32bpc resample (`Image.resize` on a mode "F" image; src/libImaging/Resample.c, ImagingResample*_32bpc): the bounds
// and the normalised fp64 coefficients of resize_coeffs_kernel BEFORE its fixed-point rounding, `double ss = 0; ss += pixel * k`
// in tap order with every operation rounded on its own (contraction off: an FMA would skip the product's rounding), float32
// between the passes, nothing clipped there.  The element type of the source and of the destination is a template parameter, so
// u16 -> resize -> u16 is two launches per pass pair and equals convert -> resize -> convert bit for bit.
// Checker: tests/resize_f32_reference.py (pinned against Pillow on the CPU); tests/test_gpu_prepost16.py.
__global__ void resize_coeffs_f64_kernel(int in_size, int out_size, int ksize, int* __restrict__ bounds, double* __restrict__ kk) {
#pragma clang fp contract(off)
    const int xx = blockIdx.x * blockDim.x + threadIdx.x;
    if (xx >= out_size) return;
    const double scale = (double)in_size / (double)out_size;
    const double filterscale = scale < 1.0 ? 1.0 : scale;
    const double support = 2.0 * filterscale;
    const double ss = 1.0 / filterscale;
    const double center = (xx + 0.5) * scale;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > in_size) xmax = in_size;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) ww += bicubic_w((x + xmin - center + 0.5) * ss);
    double* k = kk + (size_t)xx * ksize;
    for (int x = 0; x < ksize; ++x) {
        double w = 0.0;
        if (x < xmax) {
            w = bicubic_w((x + xmin - center + 0.5) * ss);
            if (ww != 0.0) w /= ww;
        }
        k[x] = w;
    }
    bounds[2 * xx] = xmin;
    bounds[2 * xx + 1] = xmax;
}

__device__ __forceinline__ float pix_load(const uint8_t* p, size_t i) { return __fdiv_rn((float)p[i], 255.0f); }
__device__ __forceinline__ float pix_load(const uint16_t* p, size_t i) { return __fdiv_rn((float)p[i], 65535.0f); }
__device__ __forceinline__ float pix_load(const float* p, size_t i) { return p[i]; }

__device__ __forceinline__ void pix_store(float* p, size_t i, float v, int clamp) {
    if (clamp) v = v < 0.f ? 0.f : (v > 1.f ? 1.f : v);
    p[i] = v;
}
__device__ __forceinline__ void pix_store(uint16_t* p, size_t i, float v, int) {
    v = !(v > 0.f) ? 0.f : (v > 1.f ? 1.f : v);                         // always clamped; a NaN stores 0
    p[i] = (uint16_t)__fadd_rn(__fmul_rn(v, 65535.0f), 0.5f);           // round to nearest: two fp32 roundings, truncation
}

// rows = n * h rows of sw pixels -> rows of dw pixels; consecutive threads: consecutive output x
template <typename S, typename D>
__global__ void resample_h_f32_kernel(const S* __restrict__ src, D* __restrict__ dst, long rows, int sw, int dw,
                                      const int* __restrict__ bounds, const double* __restrict__ kk, int ksize, int clamp) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * dw) return;
    const long row = idx / dw;
    const int xx = (int)(idx - row * dw);
    const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
    const double* k = kk + (size_t)xx * ksize;
    const size_t base = (size_t)row * sw + xmin;
    double ss = 0.0;
    for (int x = 0; x < xmax; ++x) {
        const double prod = (double)pix_load(src, base + x) * k[x];
        ss = ss + prod;
    }
    pix_store(dst, (size_t)idx, (float)ss, clamp);
}

// n images of sh x w -> dh x w; consecutive threads: consecutive x of one output row (loads and stores coalesced)
template <typename S, typename D>
__global__ void resample_v_f32_kernel(const S* __restrict__ src, D* __restrict__ dst, int n, int sh, int dh, int w,
                                      const int* __restrict__ bounds, const double* __restrict__ kk, int ksize, int clamp) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * dh * w) return;
    const int x = (int)(idx % w);
    const long t = idx / w;
    const int yy = (int)(t % dh);
    const int img = (int)(t / dh);
    const int ymin = bounds[2 * yy], ymax = bounds[2 * yy + 1];
    const double* k = kk + (size_t)yy * ksize;
    const size_t base = ((size_t)img * sh + ymin) * w + x;
    double ss = 0.0;
    for (int y = 0; y < ymax; ++y) {
        const double prod = (double)pix_load(src, base + (size_t)y * w) * k[y];
        ss = ss + prod;
    }
    pix_store(dst, (size_t)idx, (float)ss, clamp);
}

// both sizes unchanged: the pure conversion (also mi_u16_to_unit_f32 / mi_unit_f32_to_u16)
template <typename S, typename D>
__global__ void pix_convert_kernel(const S* __restrict__ src, D* __restrict__ dst, size_t count, int clamp) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) pix_store(dst, i, pix_load(src, i), clamp);
}

// workspace: [h bounds 2*dw][v bounds 2*dh] ints | [h kk dw*ksize_h][v kk dh*ksize_v] doubles | the n*sh*dw float intermediate
struct ResizeF32Layout { size_t kk_off, mid_off, total; };
static ResizeF32Layout resize_f32_layout(int n, int sw, int sh, int dw, int dh) {
    ResizeF32Layout l;
    const size_t ints = 2 * (size_t)dw + 2 * (size_t)dh;
    const size_t dbls = (size_t)dw * resize_ksize(sw, dw) + (size_t)dh * resize_ksize(sh, dh);
    l.kk_off = (ints * sizeof(int) + 255) & ~(size_t)255;
    l.mid_off = l.kk_off + ((dbls * sizeof(double) + 255) & ~(size_t)255);
    l.total = l.mid_off + (size_t)n * sh * dw * sizeof(float) + 256;
    return l;
}

size_t resize_f32_workspace_bytes(int n, int sw, int sh, int dw, int dh) { return resize_f32_layout(n, sw, sh, dw, dh).total; }

template <typename S, typename D>
static hipError_t resize_f32_typed(const S* src, int n, int sw, int sh, D* dst, int dw, int dh, int clamp, void* ws, hipStream_t s) {
    const ResizeF32Layout l = resize_f32_layout(n, sw, sh, dw, dh);
    const int kh = resize_ksize(sw, dw), kv = resize_ksize(sh, dh);
    int* hb = reinterpret_cast<int*>(ws);
    int* vb = hb + 2 * (size_t)dw;
    double* hk = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + l.kk_off);
    double* vk = hk + (size_t)dw * kh;
    float* mid = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + l.mid_off);
    const bool need_h = dw != sw, need_v = dh != sh;
    auto blocks = [](long total) { return dim3((unsigned)((total + 255) / 256)); };
    if (!need_h && !need_v) {
        const size_t count = (size_t)n * sh * sw;
        hipLaunchKernelGGL((pix_convert_kernel<S, D>), blocks((long)count), dim3(256), 0, s, src, dst, count, clamp);
        return hipGetLastError();
    }
    if (need_h) hipLaunchKernelGGL(resize_coeffs_f64_kernel, dim3((dw + 127) / 128), dim3(128), 0, s, sw, dw, kh, hb, hk);
    if (need_v) hipLaunchKernelGGL(resize_coeffs_f64_kernel, dim3((dh + 127) / 128), dim3(128), 0, s, sh, dh, kv, vb, vk);
    const long htotal = (long)n * sh * dw, vtotal = (long)n * dh * dw;
    if (need_h && need_v) {
        hipLaunchKernelGGL((resample_h_f32_kernel<S, float>), blocks(htotal), dim3(256), 0, s, src, mid, (long)n * sh, sw, dw, hb, hk, kh, 0);
        hipLaunchKernelGGL((resample_v_f32_kernel<float, D>), blocks(vtotal), dim3(256), 0, s, mid, dst, n, sh, dh, dw, vb, vk, kv, clamp);
    } else if (need_h) {
        hipLaunchKernelGGL((resample_h_f32_kernel<S, D>), blocks(htotal), dim3(256), 0, s, src, dst, (long)n * sh, sw, dw, hb, hk, kh, clamp);
    } else {
        hipLaunchKernelGGL((resample_v_f32_kernel<S, D>), blocks(vtotal), dim3(256), 0, s, src, dst, n, sh, dh, dw, vb, vk, kv, clamp);
    }
    return hipGetLastError();
}

template <typename S>
static hipError_t resize_f32_src(const S* src, int n, int sw, int sh, void* dst, int dst_type, int dw, int dh, int clamp, void* ws, hipStream_t s) {
    if (dst_type == MI_PIX_F32) return resize_f32_typed(src, n, sw, sh, static_cast<float*>(dst), dw, dh, clamp, ws, s);
    if (dst_type == MI_PIX_U16) return resize_f32_typed(src, n, sw, sh, static_cast<uint16_t*>(dst), dw, dh, clamp, ws, s);
    return hipErrorInvalidValue;
}

hipError_t resize_bicubic_f32_launch(const void* src, int src_type, int n, int sw, int sh, void* dst, int dst_type, int dw, int dh,
                                     int clamp, void* ws, hipStream_t s) {
    if (n < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1) return hipErrorInvalidValue;
    switch (src_type) {
        case MI_PIX_U8:  return resize_f32_src(static_cast<const uint8_t*>(src), n, sw, sh, dst, dst_type, dw, dh, clamp, ws, s);
        case MI_PIX_U16: return resize_f32_src(static_cast<const uint16_t*>(src), n, sw, sh, dst, dst_type, dw, dh, clamp, ws, s);
        case MI_PIX_F32: return resize_f32_src(static_cast<const float*>(src), n, sw, sh, dst, dst_type, dw, dh, clamp, ws, s);
    }
    return hipErrorInvalidValue;
}

hipError_t u16_to_unit_launch(const uint16_t* src, float* dst, size_t count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL((pix_convert_kernel<uint16_t, float>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, src, dst, count, 0);
    return hipGetLastError();
}

hipError_t unit_to_u16_launch(const float* src, uint16_t* dst, size_t count, hipStream_t s) {
    if (count == 0) return hipSuccess;
    hipLaunchKernelGGL((pix_convert_kernel<float, uint16_t>), dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, src, dst, count, 1);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ the window (include/midd.h: THE WINDOW)
// Percentile windowing of the 16-bit path: a histogram per image, the two levels from its ranks, and the element rules under those
// levels, all in integer or single-rounded fp32 arithmetic so that tests/window_reference.py restates them bit for bit.  The levels
// stay in device memory between the calls: nothing here synchronises with the host.
//
// histogram_u16_kernel: block (c, i) counts pixels [c * chunk, min((c + 1) * chunk, count)) of image i into 65536 sixteen-bit
// counters packed two per dword in LDS (128 KiB: one block per CU).  chunk <= 65535, so no counter can carry into its neighbour.
// A lane folds runs of equal values among its 8 pixels into one LDS atomic (flat regions: collimator, burnt-out air), and only the
// non-zero counters reach the [n][65536] global histogram, as integer atomics: the sums commute, the result is deterministic.
constexpr int HIST_BINS = 65536;
constexpr int HIST_THREADS = 1024;
constexpr int HIST_MAX_CHUNK = 65528;               // <= 65535 and a multiple of 8
constexpr int HIST_MIN_CHUNK = 4096;

__device__ __forceinline__ void hist_add(unsigned* lds, unsigned v, unsigned run) { atomicAdd(&lds[v >> 1], run << ((v & 1u) * 16u)); }

__global__ __launch_bounds__(HIST_THREADS)
void histogram_u16_kernel(const uint16_t* __restrict__ src, size_t count, unsigned chunk, unsigned* __restrict__ hist) {
    __shared__ uint4 lds4[HIST_BINS / 2 / 4];
    unsigned* lds = reinterpret_cast<unsigned*>(lds4);
    const unsigned tid = threadIdx.x;
    for (unsigned i = tid; i < HIST_BINS / 2 / 4; i += HIST_THREADS) lds4[i] = make_uint4(0u, 0u, 0u, 0u);
    __syncthreads();
    const size_t first = (size_t)blockIdx.x * chunk;                     // < count by the grid's size
    const unsigned len = (unsigned)(count - first < (size_t)chunk ? count - first : (size_t)chunk);
    const uint16_t* p = src + (size_t)blockIdx.y * count + first;         // 2-byte aligned only: image i starts at element i * count
    unsigned head = (unsigned)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(p) & 15u)) & 15u) >> 1);
    if (head > len) head = len;
    const unsigned vecs = (len - head) >> 3;
    const unsigned tail0 = head + (vecs << 3);
    if (tid < head) hist_add(lds, p[tid], 1u);
    if (tid < len - tail0) hist_add(lds, p[tail0 + tid], 1u);            // fewer than 8
    const uint4* pv = reinterpret_cast<const uint4*>(p + head);
    for (unsigned i = tid; i < vecs; i += HIST_THREADS) {
        const uint4 q = pv[i];
        const unsigned w[4] = {q.x, q.y, q.z, q.w};
        unsigned prev = w[0] & 0xffffu, run = 1u;
#pragma unroll
        for (int j = 1; j < 8; ++j) {
            const unsigned v = (w[j >> 1] >> ((j & 1) * 16)) & 0xffffu;
            if (v == prev) { ++run; } else { hist_add(lds, prev, run); prev = v; run = 1u; }
        }
        hist_add(lds, prev, run);
    }
    __syncthreads();
    unsigned* out = hist + (size_t)blockIdx.y * HIST_BINS;
    for (unsigned i = tid; i < HIST_BINS / 2; i += HIST_THREADS) {
        const unsigned c = lds[i];
        if (c & 0xffffu) atomicAdd(&out[2 * i], c & 0xffffu);
        if (c >> 16) atomicAdd(&out[2 * i + 1], c >> 16);
    }
}

// one block per image: thread t owns bins [64 t, 64 t + 64); an exclusive scan of the 1024 partial sums gives each thread the
// number of pixels below its bins, and the thread whose span holds rank r walks its bins to the level
constexpr int LEV_THREADS = 1024;
constexpr int LEV_BINS = HIST_BINS / LEV_THREADS;

__device__ __forceinline__ unsigned long long window_rank(double p, unsigned long long total) {
#pragma clang fp contract(off)
    const double t = p * (double)(total - 1ull);
    return (unsigned long long)floor(t / 100.0);
}

__global__ __launch_bounds__(LEV_THREADS)
void window_levels_kernel(const unsigned* __restrict__ hist, double p_lo, double p_hi, int* __restrict__ levels) {
    __shared__ unsigned long long scan[2][LEV_THREADS];
    __shared__ int found[2];
    const unsigned tid = threadIdx.x;
    const uint4* h4 = reinterpret_cast<const uint4*>(hist + (size_t)blockIdx.x * HIST_BINS + (size_t)tid * LEV_BINS);
    unsigned long long own = 0;
#pragma unroll 4
    for (int j = 0; j < LEV_BINS / 4; ++j) {
        const uint4 q = h4[j];
        own += (unsigned long long)q.x + q.y + q.z + q.w;
    }
    scan[0][tid] = own;
    __syncthreads();
    int cur = 0;
    for (unsigned off = 1; off < LEV_THREADS; off <<= 1) {               // inclusive scan, double buffered
        unsigned long long v = scan[cur][tid];
        if (tid >= off) v += scan[cur][tid - off];
        scan[cur ^ 1][tid] = v;
        cur ^= 1;
        __syncthreads();
    }
    const unsigned long long total = scan[cur][LEV_THREADS - 1];
    const unsigned long long below = scan[cur][tid] - own;
    if (total == 0) {                                                    // no pixel counted: the unwindowed rule
        if (tid == 0) { levels[2 * blockIdx.x] = 0; levels[2 * blockIdx.x + 1] = HIST_BINS - 1; }
        return;
    }
    const unsigned long long r[2] = {window_rank(p_lo, total), window_rank(p_hi, total)};
#pragma unroll
    for (int e = 0; e < 2; ++e) {
        if (below <= r[e] && r[e] < below + own) {                       // exactly one thread: r < total
            const unsigned* bins = reinterpret_cast<const unsigned*>(h4);  // read again (cached) rather than kept in 64 registers
            unsigned long long cum = below;
            int k = 0;
            for (int j = 0; j < LEV_BINS; ++j) {
                cum += bins[j];
                k += (cum <= r[e]) ? 1 : 0;                              // bins wholly at or below the rank
            }
            found[e] = (int)(tid * LEV_BINS) + k;
        }
    }
    __syncthreads();
    if (tid == 0) {
        int lo = found[0], hi = found[1];
        if (hi == lo) { if (lo < HIST_BINS - 1) hi = lo + 1; else lo = hi - 1; }
        levels[2 * blockIdx.x] = lo;
        levels[2 * blockIdx.x + 1] = hi;
    }
}

// the two element rules under a window (lo, hi), d = (float)(hi - lo)
struct Window { int lo; float d; };
__device__ __forceinline__ Window window_of(const int* __restrict__ levels, int img) {
    const int lo = levels[2 * img], hi = levels[2 * img + 1];            // img is uniform per block where it can be: scalar loads
    return Window{lo, (float)(hi - lo)};
}
__device__ __forceinline__ float win_load(uint16_t v, Window w) {
    const float x = __fdiv_rn((float)((int)v - w.lo), w.d);              // the integer difference is exact in fp32
    return x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
}
__device__ __forceinline__ uint16_t win_store(float v, Window w) {
    v = !(v > 0.f) ? 0.f : (v > 1.f ? 1.f : v);                          // a NaN stores lo
    return (uint16_t)((unsigned)w.lo + (unsigned)__fadd_rn(__fmul_rn(v, w.d), 0.5f));
}

// element access of the windowed resample: the windowed rule for a u16 side, the plain one for every other type
__device__ __forceinline__ float wpix_load(const uint8_t* p, size_t i, Window) { return pix_load(p, i); }
__device__ __forceinline__ float wpix_load(const float* p, size_t i, Window) { return pix_load(p, i); }
__device__ __forceinline__ float wpix_load(const uint16_t* p, size_t i, Window w) { return win_load(p[i], w); }
__device__ __forceinline__ void wpix_store(float* p, size_t i, float v, int clamp, Window) { pix_store(p, i, v, clamp); }
__device__ __forceinline__ void wpix_store(uint16_t* p, size_t i, float v, int, Window w) { p[i] = win_store(v, w); }

// grid (x, n): image blockIdx.y of [n][count]
__global__ void window_u16_to_f32_kernel(const uint16_t* __restrict__ src, const int* __restrict__ levels, size_t count, float* __restrict__ dst) {
    const Window w = window_of(levels, blockIdx.y);
    const size_t base = (size_t)blockIdx.y * count;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        dst[base + i] = win_load(src[base + i], w);
}

__global__ void window_f32_to_u16_kernel(const float* __restrict__ src, const int* __restrict__ levels, size_t count, uint16_t* __restrict__ dst) {
    const Window w = window_of(levels, blockIdx.y);
    const size_t base = (size_t)blockIdx.y * count;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (size_t)gridDim.x * blockDim.x)
        dst[base + i] = win_store(src[base + i], w);
}

// The float resample above with a u16 side taken under the window of its image: separate instantiations, so that the unwindowed
// kernels and their bits stay what they were.  `sh`: rows per image (the horizontal pass sees n * sh rows).
template <typename S, typename D>
__global__ void resample_h_f32_window_kernel(const S* __restrict__ src, D* __restrict__ dst, long rows, int sh, int sw, int dw,
                                             const int* __restrict__ bounds, const double* __restrict__ kk, int ksize, int clamp,
                                             const int* __restrict__ levels) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * dw) return;
    const long row = idx / dw;
    const int xx = (int)(idx - row * dw);
    const Window w = window_of(levels, (int)(row / sh));
    const int xmin = bounds[2 * xx], xmax = bounds[2 * xx + 1];
    const double* k = kk + (size_t)xx * ksize;
    const size_t base = (size_t)row * sw + xmin;
    double ss = 0.0;
    for (int x = 0; x < xmax; ++x) {
        const double prod = (double)wpix_load(src, base + x, w) * k[x];
        ss = ss + prod;
    }
    wpix_store(dst, (size_t)idx, (float)ss, clamp, w);
}

template <typename S, typename D>
__global__ void resample_v_f32_window_kernel(const S* __restrict__ src, D* __restrict__ dst, int n, int sh, int dh, int w_,
                                             const int* __restrict__ bounds, const double* __restrict__ kk, int ksize, int clamp,
                                             const int* __restrict__ levels) {
#pragma clang fp contract(off)
    const long idx = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long)n * dh * w_) return;
    const int x = (int)(idx % w_);
    const long t = idx / w_;
    const int yy = (int)(t % dh);
    const int img = (int)(t / dh);
    const Window w = window_of(levels, img);
    const int ymin = bounds[2 * yy], ymax = bounds[2 * yy + 1];
    const double* k = kk + (size_t)yy * ksize;
    const size_t base = ((size_t)img * sh + ymin) * w_ + x;
    double ss = 0.0;
    for (int y = 0; y < ymax; ++y) {
        const double prod = (double)wpix_load(src, base + (size_t)y * w_, w) * k[y];
        ss = ss + prod;
    }
    wpix_store(dst, (size_t)idx, (float)ss, clamp, w);
}

// both sizes unchanged: `per_image` elements per image
template <typename S, typename D>
__global__ void pix_convert_window_kernel(const S* __restrict__ src, D* __restrict__ dst, size_t count, size_t per_image, int clamp,
                                          const int* __restrict__ levels) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const Window w = window_of(levels, (int)(i / per_image));
    wpix_store(dst, i, wpix_load(src, i, w), clamp, w);
}

template <typename S, typename D>
static hipError_t resize_f32_window_typed(const S* src, int n, int sw, int sh, D* dst, int dw, int dh, int clamp, const int* levels,
                                          void* ws, hipStream_t s) {
    const ResizeF32Layout l = resize_f32_layout(n, sw, sh, dw, dh);
    const int kh = resize_ksize(sw, dw), kv = resize_ksize(sh, dh);
    int* hb = reinterpret_cast<int*>(ws);
    int* vb = hb + 2 * (size_t)dw;
    double* hk = reinterpret_cast<double*>(reinterpret_cast<char*>(ws) + l.kk_off);
    double* vk = hk + (size_t)dw * kh;
    float* mid = reinterpret_cast<float*>(reinterpret_cast<char*>(ws) + l.mid_off);
    const bool need_h = dw != sw, need_v = dh != sh;
    auto blocks = [](long total) { return dim3((unsigned)((total + 255) / 256)); };
    if (!need_h && !need_v) {
        const size_t count = (size_t)n * sh * sw;
        hipLaunchKernelGGL((pix_convert_window_kernel<S, D>), blocks((long)count), dim3(256), 0, s, src, dst, count, (size_t)sh * sw, clamp, levels);
        return hipGetLastError();
    }
    if (need_h) hipLaunchKernelGGL(resize_coeffs_f64_kernel, dim3((dw + 127) / 128), dim3(128), 0, s, sw, dw, kh, hb, hk);
    if (need_v) hipLaunchKernelGGL(resize_coeffs_f64_kernel, dim3((dh + 127) / 128), dim3(128), 0, s, sh, dh, kv, vb, vk);
    const long htotal = (long)n * sh * dw, vtotal = (long)n * dh * dw;
    if (need_h && need_v) {      // the float intermediate has no window: the plain kernel serves a float side
        if constexpr (std::is_same<S, uint16_t>::value)
            hipLaunchKernelGGL((resample_h_f32_window_kernel<S, float>), blocks(htotal), dim3(256), 0, s, src, mid, (long)n * sh, sh, sw, dw, hb, hk, kh, 0, levels);
        else
            hipLaunchKernelGGL((resample_h_f32_kernel<S, float>), blocks(htotal), dim3(256), 0, s, src, mid, (long)n * sh, sw, dw, hb, hk, kh, 0);
        if constexpr (std::is_same<D, uint16_t>::value)
            hipLaunchKernelGGL((resample_v_f32_window_kernel<float, D>), blocks(vtotal), dim3(256), 0, s, mid, dst, n, sh, dh, dw, vb, vk, kv, clamp, levels);
        else
            hipLaunchKernelGGL((resample_v_f32_kernel<float, D>), blocks(vtotal), dim3(256), 0, s, mid, dst, n, sh, dh, dw, vb, vk, kv, clamp);
    } else if (need_h) {
        hipLaunchKernelGGL((resample_h_f32_window_kernel<S, D>), blocks(htotal), dim3(256), 0, s, src, dst, (long)n * sh, sh, sw, dw, hb, hk, kh, clamp, levels);
    } else {
        hipLaunchKernelGGL((resample_v_f32_window_kernel<S, D>), blocks(vtotal), dim3(256), 0, s, src, dst, n, sh, dh, dw, vb, vk, kv, clamp, levels);
    }
    return hipGetLastError();
}

// levels != nullptr and at least one side MI_PIX_U16 (the C ABI checks both)
hipError_t resize_bicubic_f32_window_launch(const void* src, int src_type, int n, int sw, int sh, void* dst, int dst_type, int dw, int dh,
                                            int clamp, const int* levels, void* ws, hipStream_t s) {
    if (n < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1 || !levels) return hipErrorInvalidValue;
    const bool d16 = dst_type == MI_PIX_U16;
    if (!d16 && dst_type != MI_PIX_F32) return hipErrorInvalidValue;
    uint16_t* o16 = static_cast<uint16_t*>(dst);
    float* o32 = static_cast<float*>(dst);
    switch (src_type) {
        case MI_PIX_U16:
            return d16 ? resize_f32_window_typed(static_cast<const uint16_t*>(src), n, sw, sh, o16, dw, dh, clamp, levels, ws, s)
                       : resize_f32_window_typed(static_cast<const uint16_t*>(src), n, sw, sh, o32, dw, dh, clamp, levels, ws, s);
        case MI_PIX_U8:
            if (d16) return resize_f32_window_typed(static_cast<const uint8_t*>(src), n, sw, sh, o16, dw, dh, clamp, levels, ws, s);
            break;
        case MI_PIX_F32:
            if (d16) return resize_f32_window_typed(static_cast<const float*>(src), n, sw, sh, o16, dw, dh, clamp, levels, ws, s);
            break;
    }
    return hipErrorInvalidValue;
}

static unsigned hist_chunk(int n, size_t count) {
    const size_t per_image = (size_t)((256 + n - 1) / n);               // blocks per image that fill the chip once (one block per CU)
    size_t chunk = (count + per_image - 1) / per_image;
    chunk = (chunk + 7) & ~(size_t)7;
    if (chunk < HIST_MIN_CHUNK) chunk = HIST_MIN_CHUNK;
    if (chunk > HIST_MAX_CHUNK) chunk = HIST_MAX_CHUNK;
    return (unsigned)chunk;
}

hipError_t histogram_u16_launch(const uint16_t* src, int n, size_t count, uint32_t* hist, hipStream_t s) {
    if (n < 1 || n > 65535 || count < 1 || count > 0xffffffffull) return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(hist, 0, (size_t)n * HIST_BINS * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    const unsigned chunk = hist_chunk(n, count);
    const unsigned gx = (unsigned)((count + chunk - 1) / chunk);
    hipLaunchKernelGGL(histogram_u16_kernel, dim3(gx, n), dim3(HIST_THREADS), 0, s, src, count, chunk, hist);
    return hipGetLastError();
}

hipError_t window_levels_launch(const uint32_t* hist, int n, double p_lo, double p_hi, int32_t* levels, hipStream_t s) {
    if (n < 1 || n > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_levels_kernel, dim3(n), dim3(LEV_THREADS), 0, s, hist, p_lo, p_hi, levels);
    return hipGetLastError();
}

static dim3 window_grid(int n, size_t count) {
    const size_t gx = (count + 255) / 256;
    return dim3((unsigned)(gx < 65536 ? gx : 65536), n);
}

hipError_t window_u16_to_f32_launch(const uint16_t* src, const int32_t* levels, int n, size_t count, float* dst, hipStream_t s) {
    if (n < 1 || n > 65535 || count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_u16_to_f32_kernel, window_grid(n, count), dim3(256), 0, s, src, levels, count, dst);
    return hipGetLastError();
}

hipError_t window_f32_to_u16_launch(const float* src, const int32_t* levels, int n, size_t count, uint16_t* dst, hipStream_t s) {
    if (n < 1 || n > 65535 || count < 1) return hipErrorInvalidValue;
    hipLaunchKernelGGL(window_f32_to_u16_kernel, window_grid(n, count), dim3(256), 0, s, src, levels, count, dst);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ metrics
constexpr int MET_ROWS = 4;        // image rows per block
constexpr int MET_THREADS = 256;

__device__ __forceinline__ double clamp01(float v) { return (double)(v < 0.f ? 0.f : (v > 1.f ? 1.f : v)); }

// grid (ceil(h / MET_ROWS), n): per block the squared error of its rows and the SSIM sum of its interior pixels
__global__ __launch_bounds__(MET_THREADS)
void metrics_partial_kernel(const float* __restrict__ target, const float* __restrict__ pred, int h, int w, double* __restrict__ part) {
    __shared__ double red[MET_THREADS][2];
    const int img = blockIdx.y, y0 = blockIdx.x * MET_ROWS;
    const float* t = target + (size_t)img * h * w;
    const float* p = pred + (size_t)img * h * w;
    const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03, cov_norm = 49.0 / 48.0;
    double se = 0.0, ss = 0.0;
    const int rows = min(MET_ROWS, h - y0);
    for (int i = threadIdx.x; i < rows * w; i += MET_THREADS) {
        const int y = y0 + i / w, x = i % w;
        const double a = clamp01(t[(size_t)y * w + x]), b = clamp01(p[(size_t)y * w + x]);
        se += (a - b) * (a - b);
        if (y >= 3 && y < h - 3 && x >= 3 && x < w - 3) {
            double sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
            for (int dy = -3; dy <= 3; ++dy)
                for (int dx = -3; dx <= 3; ++dx) {
                    const double u = clamp01(t[(size_t)(y + dy) * w + x + dx]), v = clamp01(p[(size_t)(y + dy) * w + x + dx]);
                    sx += u; sy += v; sxx += u * u; syy += v * v; sxy += u * v;
                }
            const double ux = sx / 49.0, uy = sy / 49.0;
            const double vx = cov_norm * (sxx / 49.0 - ux * ux), vy = cov_norm * (syy / 49.0 - uy * uy);
            const double vxy = cov_norm * (sxy / 49.0 - ux * uy);
            ss += ((2.0 * ux * uy + c1) * (2.0 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2));
        }
    }
    red[threadIdx.x][0] = se; red[threadIdx.x][1] = ss;
    __syncthreads();
    for (int off = MET_THREADS / 2; off > 0; off >>= 1) {      // fixed tree: deterministic
        if (threadIdx.x < off) { red[threadIdx.x][0] += red[threadIdx.x + off][0]; red[threadIdx.x][1] += red[threadIdx.x + off][1]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        double* o = part + ((size_t)img * gridDim.x + blockIdx.x) * 2;
        o[0] = red[0][0]; o[1] = red[0][1];
    }
}

// one thread per image: out[img] = (psnr, ssim)
__global__ void metrics_final_kernel(const double* __restrict__ part, int blocks, int n, int h, int w, double* __restrict__ out) {
    const int img = blockIdx.x * blockDim.x + threadIdx.x;
    if (img >= n) return;
    double se = 0.0, ss = 0.0;
    for (int i = 0; i < blocks; ++i) { se += part[((size_t)img * blocks + i) * 2]; ss += part[((size_t)img * blocks + i) * 2 + 1]; }
    const double mse = se / ((double)h * w);
    out[2 * img] = 10.0 * log10(1.0 / mse);
    out[2 * img + 1] = ss / ((double)(h - 6) * (w - 6));
}

size_t metrics_workspace_bytes(int n, int h) { return (size_t)n * ((h + MET_ROWS - 1) / MET_ROWS) * 2 * sizeof(double) + 256; }

hipError_t metrics_launch(const float* target, const float* pred, int n, int h, int w, double* out, void* ws, hipStream_t s) {
    if (n < 1 || h < 7 || w < 7) return hipErrorInvalidValue;       // the 7x7 SSIM window must fit (skimage raises too)
    const int blocks = (h + MET_ROWS - 1) / MET_ROWS;
    double* part = reinterpret_cast<double*>(ws);
    hipLaunchKernelGGL(metrics_partial_kernel, dim3(blocks, n), dim3(MET_THREADS), 0, s, target, pred, h, w, part);
    hipLaunchKernelGGL(metrics_final_kernel, dim3((n + 63) / 64), dim3(64), 0, s, part, blocks, n, h, w, out);
    return hipGetLastError();
}

}  // namespace midd
