// The noise power spectrum of a field f = a - b (include/midd.h: THE NOISE POWER SPECTRUM; tests/nps_reference.py restates it in
// numpy): Welch's method over overlapping R x R regions of interest (ROIs) -- detrend, window, 2-D DFT in fp32, |F|^2 in double,
// averaged over the ROIs of a group (b, c) and binned by radial frequency.  The stages are those of nps_common.h; what is this unit's:
//   nps_roi_kernel<R>  256 lanes.  f = a - b is ONE real field: the lane keeps its row quads and, for the row sums, puts them into the
//                      imaginary slots in natural order; R lanes add a row each, lane 0 forms m, ax, ay; the element is written as
//                      (d, 0).  The column pass covers the columns 0 .. R/2 only (the row transform of real data is Hermitian; the
//                      other columns follow by P[v][u] = P[(R - v) % R][R - u]).  The lane owns the entries idx = lane + 256 e of the
//                      half plane [R][R/2 + 1] and adds P = re^2 + im^2.  LDS: 8.7 KiB, 33.7 KiB and 131.7 KiB for R = 32, 64, 128
//   nps_sum_kernel<R>  64 loads in flight, the scale, the entry and its mirror
#include <cmath>
#include "nps_common.h"

#pragma clang fp contract(off)

namespace midd {

// grid (chunks, groups); part [G][chunks][HALF] doubles, used [G][chunks]
template <int R>
__global__ __launch_bounds__(NPS_THREADS)
void nps_roi_kernel(const float* __restrict__ a, const float* __restrict__ b, int K, int C, int H, int W, int S, int ny, int nx,
                    unsigned long long n_rois, int detrend, int windowed, NpsTables tab, double* __restrict__ part, long long* __restrict__ used) {
    using G = NpsGeom<R>;
    constexpr int LOG = G::LOG, NC = G::NC, P = G::P, HALF = G::HALF, NACC = G::NACC;
    constexpr int COLT = ((NC * (R / 2) + NPS_THREADS - 1) / NPS_THREADS + 1) / 2 * 2;      // column-pass trips per lane, made even: 2, 6, 18
    constexpr int NQ = R * R / 4 / NPS_THREADS;                          // row quads per lane: 1, 4, 16
    __shared__ float2 z[R * P];                                          // (re, im), pitch R + 1
    __shared__ float2 tw[R / 2];
    __shared__ float win[R];
    __shared__ double rs0[R], rs1[R];
    __shared__ double coef[3];
    __shared__ int bad;
    const int tid = threadIdx.x;
    const unsigned chunk = blockIdx.x, chunks = gridDim.x;
    const size_t g = blockIdx.y;
    const size_t bi = g / (unsigned)C, c = g % (unsigned)C;
    const size_t plane = (size_t)H * W;
    if (tid < R / 2) tw[tid] = make_float2(tab.tc[tid], tab.ts[tid]);
    if (tid < R) win[tid] = tab.w[tid];
    double acc[NACC];
#pragma unroll
    for (int e = 0; e < NACC; ++e) acc[e] = 0.0;
    long long n_used = 0;
    NpsWalk w = nps_walk(chunk, n_rois, ny, nx);
#pragma unroll 1
    for (unsigned long long r = w.r0; r < w.r1; ++r, ++w.rem) {
        size_t oy, ox;
        nps_walk_roi(w, nx, S, oy, ox);
        const float* pa = a + ((bi * K + w.m) * C + c) * plane + oy * W + ox;
        const float* pb = b ? b + (bi * C + c) * plane + oy * W + ox : nullptr;
        if (tid == 0) bad = 0;
        __syncthreads();
        // f = a - b: the lane keeps its quads; with a detrend they also go to the imaginary slots, in natural order, for the row sums
        f32x4 fq[NQ];
        {
            const bool wide = (W & 3) == 0;
            if (wide && nps_aligned16(pa)) nps_load_quads<R, NQ, 4>(pa, (size_t)W, tid, fq);
            else nps_load_quads<R, NQ, 1>(pa, (size_t)W, tid, fq);
            if (pb) {
                f32x4 sub[NQ];
                if (wide && nps_aligned16(pb)) nps_load_quads<R, NQ, 4>(pb, (size_t)W, tid, sub);
                else nps_load_quads<R, NQ, 1>(pb, (size_t)W, tid, sub);
#pragma unroll
                for (int e = 0; e < NQ; ++e) fq[e] = (f32x4){fq[e].x - sub[e].x, fq[e].y - sub[e].y, fq[e].z - sub[e].z, fq[e].w - sub[e].w};
            }
        }
        bool nonfinite = false;
#pragma unroll
        for (int e = 0; e < NQ; ++e) {
            const int q = tid + NPS_THREADS * e, y = q / (R / 4), x4 = (q % (R / 4)) * 4;
            const f32x4 v = fq[e];
            nonfinite = nonfinite || !nps_finite(v.x) || !nps_finite(v.y) || !nps_finite(v.z) || !nps_finite(v.w);
            if (detrend != 0) {
                float2* dst = z + y * P + x4;
                dst[0].y = v.x; dst[1].y = v.y; dst[2].y = v.z; dst[3].y = v.w;
            }
        }
        if (nonfinite) atomicOr(&bad, 1);
        __syncthreads();
        const int skip = bad;
        if (detrend != 0 && !skip) {
            if (tid < R) {
                double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
                for (int x = 0; x < R; ++x) {
                    const double fv = (double)z[tid * P + x].y;
                    s0 = add_rn64(s0, fv);
                    s1 = add_rn64(s1, mul_rn64((double)x - 0.5 * (R - 1), fv));
                }
                rs0[tid] = s0; rs1[tid] = s1;
            }
            __syncthreads();
            if (tid == 0) {
                double t0 = 0.0, tx = 0.0, ty = 0.0;
#pragma unroll 8
                for (int y = 0; y < R; ++y) {
                    t0 = add_rn64(t0, rs0[y]);
                    tx = add_rn64(tx, rs1[y]);
                    ty = add_rn64(ty, mul_rn64((double)y - 0.5 * (R - 1), rs0[y]));
                }
                const double den = NPS_SLOPE_DEN<R>;
                coef[0] = __ddiv_rn(t0, (double)(R * R));
                coef[1] = detrend == 2 ? __ddiv_rn(tx, den) : 0.0;
                coef[2] = detrend == 2 ? __ddiv_rn(ty, den) : 0.0;
            }
        }
        __syncthreads();                      // (also: every lane has read `bad`, and the row sums have read the imaginary slots)
        if (skip) continue;
        {
            const double m0 = coef[0], ax = coef[1], ay = coef[2];
#pragma unroll
            for (int e = 0; e < NQ; ++e) {
                const int q = tid + NPS_THREADS * e, y = q / (R / 4), x4 = (q % (R / 4)) * 4;
                const float fs[4] = {fq[e].x, fq[e].y, fq[e].z, fq[e].w};
                const int yr = (int)(__brev((unsigned)y) >> (32 - LOG)) * P;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int x = x4 + i;
                    float d = fs[i];
                    if (detrend != 0) {
                        const double xc = (double)x - 0.5 * (R - 1), yc = (double)y - 0.5 * (R - 1);
                        const double t = add_rn64(add_rn64(m0, mul_rn64(ax, xc)), mul_rn64(ay, yc));
                        d = __double2float_rn(sub_rn64((double)fs[i], t));
                    }
                    if (windowed) { d = d * win[y]; d = d * win[x]; }
                    z[yr + (int)(__brev((unsigned)x) >> (32 - LOG))] = make_float2(d, 0.0f);
                }
            }
        }
        __syncthreads();
        // the rows: every row, every column
#pragma unroll 1
        for (int s = 1; s <= LOG; ++s) {
            const int half = 1 << (s - 1);
#pragma unroll 2
            for (int e = 0; e < R * R / 2 / NPS_THREADS; ++e) {             // (a constant, even trip count: the asm products are convergent)
                const int q = tid + NPS_THREADS * e, row = q % R, i = q / R;
                const int j = i & (half - 1), k = (i >> (s - 1)) << s;
                const int ia = row * P + k + j;
                nps_butterfly(z, ia, ia + half, tw[j << (LOG - s)]);
            }
            __syncthreads();
        }
        // the columns 0 .. R/2: consecutive lanes take consecutive columns
#pragma unroll 1
        for (int s = 1; s <= LOG; ++s) {
            const int half = 1 << (s - 1);
#pragma unroll 2
            for (int e = 0; e < COLT; ++e) {
                const int q = tid + NPS_THREADS * e, col = q % NC, i = q / NC;
                const int j = i & (half - 1), k = (i >> (s - 1)) << s;
                const int ia = (k + j) * P + col;
                if (q < NC * (R / 2)) nps_butterfly(z, ia, ia + half * P, tw[j << (LOG - s)]);
            }
            __syncthreads();
        }
#pragma unroll
        for (int e = 0; e < NACC; ++e) {
            const int idx = tid + NPS_THREADS * e;
            if (idx < HALF) {
                const float2 v = z[(idx / NC) * P + idx % NC];
                const double fr = (double)v.x, fi = (double)v.y;
                acc[e] = add_rn64(acc[e], add_rn64(mul_rn64(fr, fr), mul_rn64(fi, fi)));
            }
        }
        ++n_used;
        __syncthreads();                      // the plane is written again by the next ROI
    }
    double* dst = part + (g * chunks + chunk) * (size_t)HALF;
#pragma unroll
    for (int e = 0; e < NACC; ++e) {
        const int idx = tid + NPS_THREADS * e;
        if (idx < HALF) dst[idx] = acc[e];
    }
    if (tid == 0) used[g * chunks + chunk] = n_used;
}

// grid (ceil(HALF / 64), groups): the chunk sums of one entry (nps_chunk_sum), scaled
constexpr int NPS_SUM_THREADS = 64;
constexpr int NPS_SUM_BATCH = 64;
template <int R>
__global__ __launch_bounds__(NPS_SUM_THREADS)
void nps_sum_kernel(const double* __restrict__ part, const long long* __restrict__ used, unsigned chunks, unsigned long long n_rois,
                    double scale, double sw, double* __restrict__ nps, long long* __restrict__ rois_used, long long* __restrict__ rois_skipped) {
    constexpr int HALF = NpsGeom<R>::HALF;
    const size_t g = blockIdx.y;
    const int idx = blockIdx.x * NPS_SUM_THREADS + threadIdx.x;
    // the used ROIs of the group: integers, so the order is free -- a strided share per lane, folded over the wave
    long long n = 0;
#pragma unroll 8
    for (unsigned c = threadIdx.x; c < chunks; c += NPS_SUM_THREADS) n += used[g * chunks + c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (idx == 0) { rois_used[g] = n; rois_skipped[g] = (long long)n_rois - n; }
    if (idx >= HALF) return;
    const double s = nps_chunk_sum<NPS_SUM_BATCH, HALF>(part + g * chunks * (size_t)HALF + idx, chunks);
    const double val = n > 0 ? __ddiv_rn(mul_rn64(scale, s), mul_rn64((double)n, sw)) : __longlong_as_double((long long)NPS_QNAN);
    nps_store_mirrored<R>(nps, 0, 0, g, idx, val, val);
}

// ---------------------------------------------------------------------------------------------------------------- launches
unsigned long long nps_chunks(int K, int H, int W, int R, int S) { return nps_counts(K, H, W, R, S).chunks; }

size_t nps_workspace_bytes(int groups, int K, int H, int W, int R, int S) {
    return (size_t)groups * nps_chunks(K, H, W, R, S) * ((size_t)R * (R / 2 + 1) + 1) * sizeof(double);
}

// the tables: twiddles exp(-2 pi i t / R), t < R/2, and the window, computed in double and rounded to fp32; S_w = (sum w^2)^2
void nps_tables(int R, const float* window, NpsTables* tab, double* sw) {
    for (int t = 0; t < R / 2; ++t) {
        const double ang = 2.0 * M_PI * (double)t / (double)R;
        tab->tc[t] = (float)cos(ang);
        tab->ts[t] = (float)-sin(ang);
    }
    *sw = (double)R * (double)R;
    if (window) {
        double q = 0.0;
        for (int i = 0; i < R; ++i) { tab->w[i] = window[i]; q += (double)window[i] * (double)window[i]; }
        *sw = q * q;
    }
}

// (every argument has been judged by the entry, mi_noise_power_spectrum, with a message)
hipError_t nps_launch(const float* a, const float* b, int B, int K, int C, int H, int W, int R, int S, int detrend, const float* window,
                      double scale, int exclude_axes, double* nps, double* radial, long long* radial_count, long long* rois_used,
                      long long* rois_skipped, void* ws, hipStream_t s) {
    NpsTables tab{};
    double sw;
    nps_tables(R, window, &tab, &sw);
    const int groups = B * C, windowed = window ? 1 : 0;
    const NpsCounts n = nps_counts(K, H, W, R, S);
    const unsigned chunks = (unsigned)n.chunks;
    double* part = static_cast<double*>(ws);
    return nps_for_roi_size(R, [&](auto size) {
        constexpr int N = decltype(size)::value;
        using G = NpsGeom<N>;
        long long* used = reinterpret_cast<long long*>(part + (size_t)groups * chunks * G::HALF);
        hipLaunchKernelGGL((nps_roi_kernel<N>), dim3(chunks, groups), dim3(NPS_THREADS), 0, s, a, b, K, C, H, W, S, n.ny, n.nx, n.n_rois, detrend,
                           windowed, tab, part, used);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((nps_sum_kernel<N>), dim3((G::HALF + NPS_SUM_THREADS - 1) / NPS_SUM_THREADS, groups), dim3(NPS_SUM_THREADS), 0, s, part,
                           used, chunks, n.n_rois, scale, sw, nps, rois_used, rois_skipped);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((nps_radial_kernel<N>), dim3((N / 2 + 1 + 3) / 4, groups), dim3(NPS_THREADS), 0, s, nps, rois_used, exclude_axes, radial,
                           radial_count);
        return hipGetLastError();
    });
}

}  // namespace midd
