// The Welch cross-spectrum of two fields x and y (include/midd.h: THE CROSS SPECTRUM; tests/cross_spectrum_reference.py restates it
// in numpy).  The stages are those of nps_common.h; here ONE complex transform per ROI carries both fields, z = (dx, dy), and four
// double spectra follow from Z[v][u] and Z[-v][-u].  What is this unit's:
//   xs_roi_kernel<R>   T = 256 lanes (512 at R = 128, where four accumulators per entry and two fields' quads at 256 lanes would pass
//                      the register file).  A non-finite value in either field skips the ROI; lanes 0 .. R-1 add the rows of x while
//                      lanes R .. 2R-1 add those of y, lanes 0 and 64 form the two sets of coefficients, behind the same barriers.
//                      The column pass covers all R columns (the rows of a complex field are not Hermitian).  The lane owns the
//                      half-plane entries of XsGeom, reads Z1 = Z[v][u] and Z2 = Z[(R-v)%R][(R-u)%R] and adds Sxx, Syy, Re Sxy,
//                      Im Sxy.  At R = 128 the quads are not kept across the detrend sums but loaded again, four per field at a time
//   xs_sum_kernel<R>   one lane per (quantity, entry): 32 loads in flight, the division, the mirror (Im Sxy with the opposite sign)
//   nps_radial_kernel<R>   once per quantity
#include <cmath>
#include "nps_common.h"

#pragma clang fp contract(off)

namespace midd {

template <int R> struct XsGeom {
    static constexpr int T = R == 128 ? 512 : 256;                          // lanes per workgroup
    static constexpr int NQ = R * R / 4 / T;                                 // row quads per lane and field: 1, 4, 8
    static constexpr bool KEEP = R < 128;                                    // the quads stay in registers across the detrend sums
    static constexpr int NB = KEEP ? NQ : 4;                                 // quads per batch
    // the lane's half-plane entries: column u0 = lane % (R/2) at the rows v0 + VS e, v0 = lane / (R/2), and, for the lanes below R,
    // one entry (lane, R/2) of the last column: addresses with a constant stride, which need no division and no register each
    static constexpr int VS = T / (R / 2);                                   // 16, 8, 8
    static constexpr int NACC = R / VS + 1;                                  // 3, 9, 17
    static constexpr int BFLY = R * R / 2 / T;                               // butterflies per lane and stage: 2, 8, 16
};

// grid (chunks, groups); part [G][chunks][4][HALF] doubles, used [G][chunks].  sx, sy: the member stride in planes of C images (0: the
// field has one realisation, broadcast over the K members)
template <int R>
__global__ __launch_bounds__(XsGeom<R>::T)
void xs_roi_kernel(const float* __restrict__ x, const float* __restrict__ y, int Kx, int Ky, int C, int H, int W, int S, int ny, int nx,
                   unsigned long long n_rois, int detrend, int windowed, NpsTables tab, double* __restrict__ part, long long* __restrict__ used) {
    using G = NpsGeom<R>;
    using X = XsGeom<R>;
    constexpr int LOG = G::LOG, NC = G::NC, P = G::P, HALF = G::HALF, T = X::T, NQ = X::NQ, NB = X::NB, NACC = X::NACC;
    static_assert(2 * R <= T && X::BFLY % 2 == 0, "two sets of row sums; an even butterfly trip count");
    __shared__ float2 z[R * P];                                          // (re, im), pitch R + 1
    __shared__ float2 tw[R / 2];
    __shared__ float win[R];
    __shared__ double rs0[2][R], rs1[2][R];
    __shared__ double coef[2][3];
    __shared__ int bad;
    constexpr int VS = X::VS;
    const int tid = threadIdx.x, u0 = tid % (R / 2), v0 = tid / (R / 2);
    const unsigned chunk = blockIdx.x, chunks = gridDim.x;
    const size_t g = blockIdx.y;
    const size_t bi = g / (unsigned)C, c = g % (unsigned)C;
    const size_t plane = (size_t)H * W;
    const size_t sx = Kx > 1 ? 1 : 0, sy = Ky > 1 ? 1 : 0;
    if (tid < R / 2) tw[tid] = make_float2(tab.tc[tid], tab.ts[tid]);
    if (tid < R) win[tid] = tab.w[tid];
    double axx[NACC], ayy[NACC], are[NACC], aim[NACC];
#pragma unroll
    for (int e = 0; e < NACC; ++e) { axx[e] = 0.0; ayy[e] = 0.0; are[e] = 0.0; aim[e] = 0.0; }
    long long n_used = 0;
    NpsWalk w = nps_walk(chunk, n_rois, ny, nx);
#pragma unroll 1
    for (unsigned long long r = w.r0; r < w.r1; ++r, ++w.rem) {
        size_t oy, ox;
        nps_walk_roi(w, nx, S, oy, ox);
        const float* px = x + ((bi * Kx + w.m * sx) * C + c) * plane + oy * W + ox;
        const float* py = y + ((bi * Ky + w.m * sy) * C + c) * plane + oy * W + ox;
        if (tid == 0) bad = 0;
        __syncthreads();
        const bool wide = (W & 3) == 0;
        const bool widex = wide && nps_aligned16(px), widey = wide && nps_aligned16(py);
        // batch e0 of a lane's quads, NB per field.  KEEP: one batch, which stays in registers until it is detrended; otherwise the
        // batches are loaded a second time there (the ROI was just read: the loads hit in the cache and give the same values)
        // (the lane index is made opaque per ROI: what follows from it -- quad positions, centred coordinates, window factors -- is
        // then formed where it is used and not once before the ROI loop, at the cost of a register each for the whole kernel)
        f32x4 xq[NB], yq[NB];
        int lt = tid;
        asm volatile("" : "+v"(lt));
        auto load = [&](int e0) {
            if (widex) nps_load_quads<R, NB, 4, T>(px, (size_t)W, lt + T * e0, xq);
            else nps_load_quads<R, NB, 1, T>(px, (size_t)W, lt + T * e0, xq);
            if (widey) nps_load_quads<R, NB, 4, T>(py, (size_t)W, lt + T * e0, yq);
            else nps_load_quads<R, NB, 1, T>(py, (size_t)W, lt + T * e0, yq);
        };
        bool nonfinite = false;
#pragma unroll 1
        for (int e0 = 0; e0 < NQ; e0 += NB) {
            load(e0);
#pragma unroll
            for (int e = 0; e < NB; ++e) {
                const int q = lt + T * (e0 + e), yy = q / (R / 4), x4 = (q % (R / 4)) * 4;
                const f32x4 a = xq[e], b = yq[e];
                nonfinite = nonfinite || !nps_finite(a.x) || !nps_finite(a.y) || !nps_finite(a.z) || !nps_finite(a.w) ||
                            !nps_finite(b.x) || !nps_finite(b.y) || !nps_finite(b.z) || !nps_finite(b.w);
                if (detrend != 0) {                                      // natural order, for the row sums
                    float2* dst = z + yy * P + x4;
                    dst[0] = make_float2(a.x, b.x); dst[1] = make_float2(a.y, b.y); dst[2] = make_float2(a.z, b.z); dst[3] = make_float2(a.w, b.w);
                }
            }
        }
        if (nonfinite) atomicOr(&bad, 1);
        __syncthreads();
        const int skip = bad;
        if (detrend != 0 && !skip) {
            if (tid < 2 * R) {                                           // lanes 0 .. R-1: the rows of x; R .. 2R-1: the rows of y
                const int f = tid / R, row = tid % R;
                double s0 = 0.0, s1 = 0.0;
#pragma unroll 8
                for (int xx = 0; xx < R; ++xx) {
                    const float2 e = z[row * P + xx];
                    const double fv = (double)(f ? e.y : e.x);
                    s0 = add_rn64(s0, fv);
                    s1 = add_rn64(s1, mul_rn64((double)xx - 0.5 * (R - 1), fv));
                }
                rs0[f][row] = s0; rs1[f][row] = s1;
            }
            __syncthreads();
            if (tid == 0 || tid == 64) {
                const int f = tid >> 6;
                double t0 = 0.0, tx = 0.0, ty = 0.0;
#pragma unroll 8
                for (int yy = 0; yy < R; ++yy) {
                    t0 = add_rn64(t0, rs0[f][yy]);
                    tx = add_rn64(tx, rs1[f][yy]);
                    ty = add_rn64(ty, mul_rn64((double)yy - 0.5 * (R - 1), rs0[f][yy]));
                }
                const double den = NPS_SLOPE_DEN<R>;
                coef[f][0] = __ddiv_rn(t0, (double)(R * R));
                coef[f][1] = detrend == 2 ? __ddiv_rn(tx, den) : 0.0;
                coef[f][2] = detrend == 2 ? __ddiv_rn(ty, den) : 0.0;
            }
        }
        __syncthreads();                      // (also: every lane has read `bad`, and the row sums have read the plane)
        if (skip) continue;
        {
            asm volatile("" : "+v"(lt));
            const double mx = coef[0][0], axc = coef[0][1], ayc = coef[0][2];
            const double my = coef[1][0], bxc = coef[1][1], byc = coef[1][2];
#pragma unroll 1
            for (int e0 = 0; e0 < NQ; e0 += NB) {
                if constexpr (!X::KEEP) load(e0);
#pragma unroll
                for (int e = 0; e < NB; ++e) {
                    const int q = lt + T * (e0 + e), yy = q / (R / 4), x4 = (q % (R / 4)) * 4;
                    const float fx[4] = {xq[e].x, xq[e].y, xq[e].z, xq[e].w};
                    const float fy[4] = {yq[e].x, yq[e].y, yq[e].z, yq[e].w};
                    const int yr = (int)(__brev((unsigned)yy) >> (32 - LOG)) * P;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const int xx = x4 + i;
                        float dx = fx[i], dy = fy[i];
                        if (detrend != 0) {
                            const double xc = (double)xx - 0.5 * (R - 1), yc = (double)yy - 0.5 * (R - 1);
                            const double tx = add_rn64(add_rn64(mx, mul_rn64(axc, xc)), mul_rn64(ayc, yc));
                            const double ty = add_rn64(add_rn64(my, mul_rn64(bxc, xc)), mul_rn64(byc, yc));
                            dx = __double2float_rn(sub_rn64((double)fx[i], tx));
                            dy = __double2float_rn(sub_rn64((double)fy[i], ty));
                        }
                        if (windowed) { dx = dx * win[yy]; dx = dx * win[xx]; dy = dy * win[yy]; dy = dy * win[xx]; }
                        z[yr + (int)(__brev((unsigned)xx) >> (32 - LOG))] = make_float2(dx, dy);
                    }
                }
            }
        }
        __syncthreads();
        // the rows
#pragma unroll 1
        for (int s = 1; s <= LOG; ++s) {
            const int half = 1 << (s - 1);
#pragma unroll 2
            for (int e = 0; e < X::BFLY; ++e) {                          // (a constant, even trip count: the asm products are convergent)
                const int q = tid + T * e, row = q % R, i = q / R;
                const int j = i & (half - 1), k = (i >> (s - 1)) << s;
                const int ia = row * P + k + j;
                nps_butterfly(z, ia, ia + half, tw[j << (LOG - s)]);
            }
            __syncthreads();
        }
        // the columns, all R of them: consecutive lanes take consecutive columns
#pragma unroll 1
        for (int s = 1; s <= LOG; ++s) {
            const int half = 1 << (s - 1);
#pragma unroll 2
            for (int e = 0; e < X::BFLY; ++e) {
                const int q = tid + T * e, col = q % R, i = q / R;
                const int j = i & (half - 1), k = (i >> (s - 1)) << s;
                const int ia = (k + j) * P + col;
                nps_butterfly(z, ia, ia + half * P, tw[j << (LOG - s)]);
            }
            __syncthreads();
        }
        // the separation: X = (Z1 + conj Z2) / 2, Y = (Z1 - conj Z2) / (2i); products of fp32 values are exact in double
        // Z1 at i1 + VS P e and, from the second entry on, Z2 at i2 - VS P e (their rows R - v0 - VS e lie in 1 .. R-1): one
        // addition each.  The two bases are made opaque here so that the per-entry addresses are formed where they are used and
        // not once before the ROI loop, where they would cost a register each for the whole kernel
        int i1 = v0 * P + u0, i2 = (R - v0) * P + ((R - u0) & (R - 1));
        asm volatile("" : "+v"(i1), "+v"(i2));
#pragma unroll
        for (int e = 0; e < NACC; ++e) {
            const bool last = e == NACC - 1;                             // the entry (lane, R/2) of the lanes below R
            const int a1 = last ? tid * P + R / 2 : i1 + VS * P * e;
            const int a2 = last ? ((R - tid) & (R - 1)) * P + R / 2 : e == 0 ? (v0 == 0 ? i2 - R * P : i2) : i2 - VS * P * e;
            if (!last || tid < R) {
                const float2 z1 = z[a1], z2 = z[a2];
                const double x1 = (double)z1.x, y1 = (double)z1.y, x2 = (double)z2.x, y2 = (double)z2.y;
                const double n1 = add_rn64(mul_rn64(x1, x1), mul_rn64(y1, y1)), n2 = add_rn64(mul_rn64(x2, x2), mul_rn64(y2, y2));
                const double cc = sub_rn64(mul_rn64(x1, x2), mul_rn64(y1, y2)), ss = add_rn64(mul_rn64(x1, y2), mul_rn64(y1, x2));
                const double nn = add_rn64(n1, n2), c2 = mul_rn64(2.0, cc);
                axx[e] = add_rn64(axx[e], mul_rn64(add_rn64(nn, c2), 0.25));
                ayy[e] = add_rn64(ayy[e], mul_rn64(sub_rn64(nn, c2), 0.25));
                are[e] = add_rn64(are[e], mul_rn64(ss, 0.5));
                aim[e] = add_rn64(aim[e], mul_rn64(sub_rn64(n1, n2), 0.25));
            }
        }
        ++n_used;
        __syncthreads();                      // the plane is written again by the next ROI
    }
    double* dst = part + (g * chunks + chunk) * (size_t)(4 * HALF);
#pragma unroll
    for (int e = 0; e < NACC; ++e) {
        const int v = e < NACC - 1 ? v0 + VS * e : tid, u = e < NACC - 1 ? u0 : R / 2;
        const int idx = v * NC + u;
        if (e < NACC - 1 || tid < R) { dst[idx] = axx[e]; dst[HALF + idx] = ayy[e]; dst[2 * HALF + idx] = are[e]; dst[3 * HALF + idx] = aim[e]; }
    }
    if (tid == 0) used[g * chunks + chunk] = n_used;
}

// grid (ceil(HALF / 64), groups, 4 quantities): the chunk sums of one entry of one quantity, one by one from 0 in chunk order
constexpr int XS_SUM_THREADS = 64;
constexpr int XS_SUM_BATCH = 32;
template <int R>
__global__ __launch_bounds__(XS_SUM_THREADS)
void xs_sum_kernel(const double* __restrict__ part, const long long* __restrict__ used, unsigned chunks, unsigned long long n_rois,
                   double sw, double* __restrict__ planes, long long* __restrict__ rois_used, long long* __restrict__ rois_skipped) {
    using G = NpsGeom<R>;
    constexpr int HALF = G::HALF;
    const size_t g = blockIdx.y, groups = gridDim.y, qty = blockIdx.z;
    const int idx = blockIdx.x * XS_SUM_THREADS + threadIdx.x;
    long long n = 0;
#pragma unroll 8
    for (unsigned c = threadIdx.x; c < chunks; c += XS_SUM_THREADS) n += used[g * chunks + c];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
    if (idx == 0 && qty == 0) { rois_used[g] = n; rois_skipped[g] = (long long)n_rois - n; }
    if (idx >= HALF) return;
    const double s = nps_chunk_sum<XS_SUM_BATCH, (size_t)4 * HALF>(part + (g * chunks * 4 + qty) * (size_t)HALF + idx, chunks);
    const double qnan = __longlong_as_double((long long)NPS_QNAN);
    const double val = n > 0 ? __ddiv_rn(s, mul_rn64((double)n, sw)) : qnan;
    nps_store_mirrored<R>(planes, qty, groups, g, idx, val, (qty == 3 && n > 0) ? -val : val);      // Sxy(-f) = conj Sxy(f)
}

// ---------------------------------------------------------------------------------------------------------------- launches
size_t xs_workspace_bytes(int groups, int K, int H, int W, int R, int S) {
    return (size_t)groups * nps_chunks(K, H, W, R, S) * (4 * (size_t)R * (R / 2 + 1) + 1) * sizeof(double);
}

// (every argument has been judged by the entry, mi_cross_spectrum, with a message)
hipError_t xs_launch(const float* x, const float* y, int B, int Kx, int Ky, int C, int H, int W, int R, int S, int detrend, const float* window,
                     int exclude_axes, double* planes, double* radial, long long* radial_count, long long* rois_used, long long* rois_skipped,
                     void* ws, hipStream_t s) {
    NpsTables tab{};
    double sw;
    nps_tables(R, window, &tab, &sw);
    const int groups = B * C, windowed = window ? 1 : 0;
    const NpsCounts n = nps_counts(Kx > Ky ? Kx : Ky, H, W, R, S);
    const unsigned chunks = (unsigned)n.chunks;
    double* part = static_cast<double*>(ws);
    return nps_for_roi_size(R, [&](auto size) {
        constexpr int N = decltype(size)::value;
        using G = NpsGeom<N>;
        long long* used = reinterpret_cast<long long*>(part + (size_t)groups * chunks * 4 * G::HALF);
        hipLaunchKernelGGL((xs_roi_kernel<N>), dim3(chunks, groups), dim3(XsGeom<N>::T), 0, s, x, y, Kx, Ky, C, H, W, S, n.ny, n.nx, n.n_rois, detrend,
                           windowed, tab, part, used);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL((xs_sum_kernel<N>), dim3((G::HALF + XS_SUM_THREADS - 1) / XS_SUM_THREADS, groups, 4), dim3(XS_SUM_THREADS), 0, s, part,
                           used, chunks, n.n_rois, sw, planes, rois_used, rois_skipped);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        for (int q = 0; q < 4; ++q) {
            hipLaunchKernelGGL((nps_radial_kernel<N>), dim3((N / 2 + 1 + 3) / 4, groups), dim3(NPS_THREADS), 0, s, planes + (size_t)q * groups * N * N,
                               rois_used, exclude_axes, radial + (size_t)q * groups * (N / 2 + 1), radial_count);
            e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    });
}

}  // namespace midd
