// Proper scores of an ensemble against a truth image (include/midd.h: THE ENSEMBLE SCORES; tests/ensemble_scores_reference.py
// restates it in numpy): per pixel the CRPS of the members' empirical distribution, the squared error of their mean, their unbiased
// variance, the mid-rank of the truth among them and whether the truth lies below each of up to 8 quantiles -- and per image the
// double sums, the rank histogram and the level counts of those.
//   ensemble_scores_kernel<KP, V>   a workgroup of 256 lanes walks chunks of 1024 consecutive elements of ONE image; lane j owns elements
//                                   4j .. 4j+3 of the chunk.  V = 4: one 16-byte load per member brings the lane's four pixels (chw a
//                                   multiple of 4, every pointer 16-byte aligned), their K x 4 values stay in registers and the pixels are
//                                   scored one after the other, each sorted in place once its member-order sums are taken.  V = 1: the
//                                   same four pixels one at a time with 4-byte loads, whatever the alignment.  Both run score_pixel, so
//                                   they agree bit for bit.  Every member is read once.
//                                   The lane adds its four pixels in element order from 0, the 256 lane sums are folded by the fixed tree
//                                   v[j] += v[j + off], off = 128 .. 1, and the chunk's four sums go to the workspace: no floating-point
//                                   atomics, and nothing of the launch geometry in the order.  The integers (rank histogram, level counts,
//                                   invalid pixels) are counted in LDS over all the chunks of the workgroup -- the level counts and the
//                                   invalid pixels as one wave ballot each -- and the non-zero counters are added to the outputs with
//                                   64-bit integer atomics: those sums commute.
//   ensemble_scores_zero_kernel     the call's integer outputs, zeroed on the stream in one launch
//   ensemble_scores_final_kernel    one thread per (image, quantity) adds the image's chunk sums one by one from 0 in chunk order
// The keys never leave the registers: the sort network and the order-statistic pick of quantile_common.h, no run-time register index
// (tests/test_ensemble_scores_cpu.py holds every instantiation to a private segment of 0 bytes).  Contraction is off for the whole
// unit; the sums and products go through the *_rn64 helpers of pointwise_common.h, the divisions are the correctly rounded ones.
#include "midd_internal.h"
#include "quantile_common.h"

#pragma clang fp contract(off)

namespace midd {

constexpr int SCORES_THREADS = 256;
constexpr int SCORES_CHUNK = 4 * SCORES_THREADS;                      // 1024: the unit of the summation order (include/midd.h)
static_assert(SCORES_CHUNK == 1024, "THE ENSEMBLE SCORES: chunks of 1024 elements, four per lane");
// the workgroup's counters in LDS: the rank bins 0 .. 2K, then (lt, le) per level, then the invalid pixels
constexpr int SCORES_RANK_BINS = 2 * QUANTILE_MAX_MEMBERS + 1;        // 129
constexpr int SCORES_CNT_LEVELS = SCORES_RANK_BINS;
constexpr int SCORES_CNT_INVALID = SCORES_CNT_LEVELS + 2 * QUANTILE_MAX_LEVELS;
constexpr int SCORES_COUNTERS = SCORES_CNT_INVALID + 1;               // 146
constexpr unsigned SCORES_MAX_GROUPS = 4096;                          // workgroups of a launch, about: more chunks than that are walked in turns

__device__ __forceinline__ bool is_finite_bits(uint32_t bits) { return (bits & 0x7F800000u) != 0x7F800000u; }

// The member count again, as a value the compiler cannot trace back to the kernel argument.  Every `m < K` of an unrolled member
// loop is uniform and loop-invariant: left alone, the 64 masks and the 64 double coefficients of each loop are hoisted out of the
// chunk loop and held across it, which spills scalar registers by the hundred and, at KP = 64, reaches scratch.  Taken anew in front
// of each loop they live for that loop only.
__device__ __forceinline__ int uniform_again(int K) {
    asm volatile("" : "+s"(K));
    return K;
}

// one add per wave for a predicate: the counters whose address is the same in every lane
__device__ __forceinline__ void count_wave(unsigned* counter, bool pred) {
    const unsigned long long mask = __ballot(pred);
    if ((threadIdx.x & 63) == 0 && mask) atomicAdd(counter, (unsigned)__popcll(mask));
}

// One pixel of THE ENSEMBLE SCORES.  k: the bits of its K members in member order (k[K ..]: anything); they leave sorted as order keys.
// present: the element exists (the last chunk may be partial).  The integer outputs are counted here (cnt: the workgroup's counters),
// under wave-uniform control flow; the four double terms are returned for the lane's sum.
struct PixelScore { double a, g, se, var; float c; bool valid; };

template <int KP>
__device__ __forceinline__ PixelScore score_pixel(uint32_t (&k)[KP], float y, bool present, int K, const QuantileLevels& ql, unsigned* cnt) {
    const double y64 = (double)y;
    const int Ka = uniform_again(K), Kb = uniform_again(K), Kc = uniform_again(K), Kd = uniform_again(K);
    bool finite = is_finite_bits(__float_as_uint(y));
    double s = 0.0;
    int lt = 0, eq = 0;
#pragma unroll
    for (int m = 0; m < KP; ++m)
        if (m < Ka) {
            const float x = __uint_as_float(k[m]);
            finite = finite && is_finite_bits(k[m]);
            s = add_rn64(s, (double)x);
            lt += x < y ? 1 : 0;                            // float comparisons: -0.0 == +0.0
            eq += x == y ? 1 : 0;
        }
    const double mean64 = __ddiv_rn(s, (double)K);
    double v = 0.0;
#pragma unroll
    for (int m = 0; m < KP; ++m)
        if (m < Kb) {
            const double d = sub_rn64((double)__uint_as_float(k[m]), mean64);
            v = add_rn64(v, mul_rn64(d, d));
        }
    PixelScore r;
    r.var = K > 1 ? __ddiv_rn(v, (double)(K - 1)) : 0.0;
    const double dm = sub_rn64(mean64, y64);
    r.se = mul_rn64(dm, dm);
    // the member order is spent: the same registers become the keys
#pragma unroll
    for (int m = 0; m < KP; ++m) k[m] = m < Kc ? order_key(k[m]) : ORDER_KEY_PAD;
    sort_keys<KP>(k);
    double a = 0.0, g = 0.0;
#pragma unroll
    for (int i = 0; i < KP; ++i)
        if (i < Kd) {
            const double sv = (double)__uint_as_float(order_bits(k[i]));
            a = add_rn64(a, fabs(sub_rn64(sv, y64)));
            g = add_rn64(g, mul_rn64((double)(2 * i - Kd + 1), sv));       // (exact: 7 bits x 24 bits)
        }
    r.a = a;
    r.g = g;
    r.c = __double2float_rn(sub_rn64(__ddiv_rn(a, (double)K), __ddiv_rn(g, (double)(K * K))));
    r.valid = present && finite;
    if (r.valid) atomicAdd(&cnt[2 * lt + eq], 1u);
    count_wave(&cnt[SCORES_CNT_INVALID], present && !finite);
    for (int i = 0; i < ql.nq; ++i) {
        const QuantilePos p = quantile_pos(ql.q[i], K);
        const float Q = quantile_of_sorted<KP>(k, p, K, false);
        count_wave(&cnt[SCORES_CNT_LEVELS + 2 * i], r.valid && y < Q);
        count_wave(&cnt[SCORES_CNT_LEVELS + 2 * i + 1], r.valid && y <= Q);
    }
    return r;
}

// grid (workgroups per image, B); part [B][chunks][4] <- (A, G, E, V) of every chunk
template <int KP, int V>
__global__ __launch_bounds__(SCORES_THREADS)
void ensemble_scores_kernel(const float* __restrict__ samples, const float* __restrict__ truth, int K, unsigned long long chw, unsigned chunks,
                            QuantileLevels ql, double* __restrict__ part, unsigned long long* __restrict__ invalid,
                            unsigned long long* __restrict__ rank_hist, unsigned long long* __restrict__ counts, float* __restrict__ crps_map) {
    __shared__ double red[SCORES_THREADS][4];
    __shared__ unsigned cnt[SCORES_COUNTERS];
    const int tid = threadIdx.x;
    const size_t b = blockIdx.y;
    for (int i = tid; i < SCORES_COUNTERS; i += SCORES_THREADS) cnt[i] = 0u;
    __syncthreads();
    const float* src = samples + b * (size_t)K * chw;
    const float* tru = truth + b * chw;
    float* map = crps_map ? crps_map + b * chw : nullptr;
    for (unsigned chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        const unsigned long long e0 = (unsigned long long)chunk * SCORES_CHUNK + 4u * (unsigned)tid;
        double la = 0.0, lg = 0.0, le = 0.0, lv = 0.0;          // the lane's four pixels, in element order from 0
        auto add = [&](const PixelScore& r) {
            if (r.valid) { la = add_rn64(la, r.a); lg = add_rn64(lg, r.g); le = add_rn64(le, r.se); lv = add_rn64(lv, r.var); }
        };
        if constexpr (V == 4) {
            const bool present = e0 < chw;                      // (chw % 4 == 0: all four or none)
            // (four arrays and four calls, not x[4][KP] under an unrolled loop: at KP = 64 that loop stays rolled and x goes to scratch)
            uint32_t x0[KP], x1[KP], x2[KP], x3[KP];
            f32x4 yv = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
            if (present) yv = *reinterpret_cast<const f32x4*>(tru + e0);
#pragma unroll
            for (int m = 0; m < KP; ++m) {
                f32x4 xv = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                if (m < uniform_again(K) && present) xv = *reinterpret_cast<const f32x4*>(src + (size_t)m * chw + e0);
                x0[m] = __float_as_uint(xv.x); x1[m] = __float_as_uint(xv.y); x2[m] = __float_as_uint(xv.z); x3[m] = __float_as_uint(xv.w);
            }
            const float qnan = __uint_as_float(0x7FC00000u);
            const PixelScore r0 = score_pixel<KP>(x0, yv.x, present, K, ql, cnt);
            add(r0);
            const PixelScore r1 = score_pixel<KP>(x1, yv.y, present, K, ql, cnt);
            add(r1);
            const PixelScore r2 = score_pixel<KP>(x2, yv.z, present, K, ql, cnt);
            add(r2);
            const PixelScore r3 = score_pixel<KP>(x3, yv.w, present, K, ql, cnt);
            add(r3);
            if (map && present)
                *reinterpret_cast<f32x4*>(map + e0) = (f32x4){r0.valid ? r0.c : qnan, r1.valid ? r1.c : qnan, r2.valid ? r2.c : qnan, r3.valid ? r3.c : qnan};
        } else {
            for (int p = 0; p < 4; ++p) {
                const unsigned long long e = e0 + (unsigned)p;
                const bool present = e < chw;
                uint32_t x[KP];
                const float y = present ? tru[e] : 0.0f;
#pragma unroll
                for (int m = 0; m < KP; ++m) x[m] = (m < uniform_again(K) && present) ? __float_as_uint(src[(size_t)m * chw + e]) : 0u;
                const PixelScore r = score_pixel<KP>(x, y, present, K, ql, cnt);
                add(r);
                if (map && present) map[e] = r.valid ? r.c : __uint_as_float(0x7FC00000u);
            }
        }
        red[tid][0] = la; red[tid][1] = lg; red[tid][2] = le; red[tid][3] = lv;
        __syncthreads();
        for (int off = SCORES_THREADS / 2; off > 0; off >>= 1) {      // fixed tree: v[j] += v[j + off]
            if (tid < off) {
#pragma unroll
                for (int q = 0; q < 4; ++q) red[tid][q] = add_rn64(red[tid][q], red[tid + off][q]);
            }
            __syncthreads();
        }
        if (tid < 4) part[(b * chunks + chunk) * 4 + tid] = red[0][tid];
        __syncthreads();                                              // red is written again by the next chunk
    }
    // the workgroup's counters: only the non-zero ones travel, as 64-bit integer atomics
    __syncthreads();
    const int nbins = 2 * K + 1;
    for (int i = tid; i < SCORES_COUNTERS; i += SCORES_THREADS) {
        const unsigned c = cnt[i];
        if (!c) continue;
        if (i < nbins) atomicAdd(&rank_hist[b * nbins + i], (unsigned long long)c);
        else if (i >= SCORES_CNT_LEVELS && i < SCORES_CNT_LEVELS + 2 * ql.nq) atomicAdd(&counts[b * 2 * ql.nq + (i - SCORES_CNT_LEVELS)], (unsigned long long)c);
        else if (i == SCORES_CNT_INVALID) atomicAdd(&invalid[b], (unsigned long long)c);
    }
}

// one thread per (image, quantity): the image's chunk sums one by one from 0 in chunk order.  The loads of a batch do not depend on
// each other, the adds do: SCORES_FINAL_BATCH loads are in flight per step of the chain (a 2500 x 2048 image has 5000 chunk sums)
constexpr int SCORES_FINAL_BATCH = 64;
__global__ void ensemble_scores_final_kernel(const double* __restrict__ part, int B, unsigned chunks, double* __restrict__ sums) {
    const unsigned t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= (unsigned)B * 4u) return;
    const double* p = part + (size_t)(t >> 2) * chunks * 4 + (t & 3u);
    double s = 0.0;
    unsigned c = 0;
    for (; c + SCORES_FINAL_BATCH <= chunks; c += SCORES_FINAL_BATCH) {
        double v[SCORES_FINAL_BATCH];
#pragma unroll
        for (int j = 0; j < SCORES_FINAL_BATCH; ++j) v[j] = p[(size_t)(c + j) * 4];
#pragma unroll
        for (int j = 0; j < SCORES_FINAL_BATCH; ++j) s = add_rn64(s, v[j]);
    }
    for (; c < chunks; ++c) s = add_rn64(s, p[(size_t)c * 4]);
    sums[t] = s;
}

// the integer outputs of a call, zeroed by ONE launch in front of the scores kernel (three memsets cost three enqueues: at 256 x 256
// the call is its enqueues)
__global__ __launch_bounds__(SCORES_THREADS)
void ensemble_scores_zero_kernel(unsigned long long* __restrict__ invalid, size_t n_invalid, unsigned long long* __restrict__ rank_hist, size_t n_rank,
                                 unsigned long long* __restrict__ counts, size_t n_counts) {
    const size_t stride = (size_t)gridDim.x * SCORES_THREADS;
    for (size_t i = (size_t)blockIdx.x * SCORES_THREADS + threadIdx.x; i < n_invalid + n_rank + n_counts; i += stride) {
        if (i < n_invalid) invalid[i] = 0ull;
        else if (i < n_invalid + n_rank) rank_hist[i - n_invalid] = 0ull;
        else counts[i - n_invalid - n_rank] = 0ull;
    }
}

// ---------------------------------------------------------------------------------------------------------------- launches
unsigned long long ensemble_scores_chunks(unsigned long long chw) { return (chw + SCORES_CHUNK - 1) / SCORES_CHUNK; }

size_t ensemble_scores_partials_bytes(int B, unsigned long long chw) { return (size_t)B * ensemble_scores_chunks(chw) * 4 * sizeof(double); }

template <int KP>
static void ensemble_scores_dispatch(const float* samples, const float* truth, int B, int K, unsigned long long chw, const QuantileLevels& ql,
                                     double* part, unsigned long long* invalid, unsigned long long* rank_hist, unsigned long long* counts,
                                     float* crps_map, hipStream_t s) {
    const unsigned chunks = (unsigned)ensemble_scores_chunks(chw);
    // every workgroup of an image walks the same number of chunks (the last one may walk fewer)
    const unsigned cap = SCORES_MAX_GROUPS / (unsigned)B ? SCORES_MAX_GROUPS / (unsigned)B : 1u;
    const unsigned turns = (chunks + cap - 1) / cap;
    const dim3 grid((chunks + turns - 1) / turns, B);
    const bool v4 = chw % 4 == 0 && aligned16(samples) && aligned16(truth) && aligned16(crps_map);
    if (v4) hipLaunchKernelGGL((ensemble_scores_kernel<KP, 4>), grid, dim3(SCORES_THREADS), 0, s, samples, truth, K, chw, chunks, ql, part, invalid, rank_hist, counts, crps_map);
    else hipLaunchKernelGGL((ensemble_scores_kernel<KP, 1>), grid, dim3(SCORES_THREADS), 0, s, samples, truth, K, chw, chunks, ql, part, invalid, rank_hist, counts, crps_map);
}

hipError_t ensemble_scores_launch(const float* samples, const float* truth, int B, int K, unsigned long long chw, const QuantileLevels& ql,
                                  double* sums, unsigned long long* invalid, unsigned long long* rank_hist, unsigned long long* counts,
                                  float* crps_map, double* part, hipStream_t s) {
    if (B < 1 || B > 65535 || K < 1 || K > QUANTILE_MAX_MEMBERS || chw < 1 || chw >= (1ull << 32) || ql.nq < 0 || ql.nq > QUANTILE_MAX_LEVELS ||
        !samples || !truth || !sums || !invalid || !rank_hist || !part || (counts == nullptr) != (ql.nq == 0))
        return hipErrorInvalidValue;
    for (int i = 0; i < ql.nq; ++i)
        if (!(ql.q[i] >= 0.0 && ql.q[i] <= 1.0)) return hipErrorInvalidValue;
    const size_t n_invalid = (size_t)B, n_rank = (size_t)B * (2 * K + 1), n_counts = (size_t)B * ql.nq * 2;      // (counts null: n_counts == 0)
    const size_t zero_groups = (n_invalid + n_rank + n_counts + SCORES_THREADS - 1) / SCORES_THREADS;
    hipLaunchKernelGGL(ensemble_scores_zero_kernel, dim3((unsigned)(zero_groups < 1024 ? zero_groups : 1024)), dim3(SCORES_THREADS), 0, s,
                       invalid, n_invalid, rank_hist, n_rank, counts, n_counts);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (K <= 2) ensemble_scores_dispatch<2>(samples, truth, B, K, chw, ql, part, invalid, rank_hist, counts, crps_map, s);
    else if (K <= 4) ensemble_scores_dispatch<4>(samples, truth, B, K, chw, ql, part, invalid, rank_hist, counts, crps_map, s);
    else if (K <= 8) ensemble_scores_dispatch<8>(samples, truth, B, K, chw, ql, part, invalid, rank_hist, counts, crps_map, s);
    else if (K <= 16) ensemble_scores_dispatch<16>(samples, truth, B, K, chw, ql, part, invalid, rank_hist, counts, crps_map, s);
    else if (K <= 32) ensemble_scores_dispatch<32>(samples, truth, B, K, chw, ql, part, invalid, rank_hist, counts, crps_map, s);
    else ensemble_scores_dispatch<64>(samples, truth, B, K, chw, ql, part, invalid, rank_hist, counts, crps_map, s);
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ensemble_scores_final_kernel, dim3((B * 4 + 63) / 64), dim3(64), 0, s, part, B, (unsigned)ensemble_scores_chunks(chw), sums);
    return hipGetLastError();
}

}  // namespace midd
