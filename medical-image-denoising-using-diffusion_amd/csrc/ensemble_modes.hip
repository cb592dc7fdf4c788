// Principal modes of an ensemble's spread (include/midd.h: THE ENSEMBLE MODES; tests/ensemble_modes_reference.py restates it in
// numpy): the K x K Gram matrix of the centred members as a reduction over the pixels, and the projection of the centred members
// onto up to 8 weight vectors.  The eigenproblem in between is the caller's (K <= 64: a host matter).
//   ensemble_gram_small_kernel<KP, V>   K <= 8 (KP = 2, 4, 8).  A workgroup is ONE wave and walks chunks of 4096 consecutive elements
//                                       of one image: 16 rounds of 256 elements, lane j owns elements 256 r + 4 j .. + 3 of round r.
//                                       It computes the double mean itself (the members are all in its registers), centres them and
//                                       adds the KP (KP + 1) / 2 rounded products d_i * d_j to its accumulators, element after
//                                       element.  Every member is read once.
//   ensemble_mean64_kernel<V>           K > 8: the double mean of every element, once, into the workspace (8 bytes per element: what
//                                       two more members would cost a reader), the quiet NaN where a member is not finite -- a valid
//                                       mean is finite, so the NaN is the element's invalid mark -- and the count of those elements.
//   ensemble_gram_pair_kernel<V>        K > 8: the members in blocks of 8; a wave owns one pair (bi <= bj) of blocks over a chunk, i.e.
//                                       an 8 x 8 tile of G in 64 double accumulators (128 VGPRs).  It loads the 16 members of its pair
//                                       (8 on the diagonal) and the stored mean, not all K: the members are read nb times over all
//                                       pairs (nb = ceil(K / 8) blocks) instead of nb (nb + 1) / 2 times had every wave recomputed
//                                       the mean, and the mean costs the pre-pass one read of the members and 8-byte writes.
//   ensemble_gram_final_kernel          one thread per (image, i, j): the entry's chunk sums one by one from 0 in chunk order; (i, j)
//                                       and (j, i) add the same numbers in the same order, so the matrix is symmetric in its bits.
//   ensemble_project_kernel<MP, V>      per element: the mean again (every member is needed anyway), then the members a second time
//                                       (they come from the cache) against M weight rows, M <= MP accumulators per element.
// V = 4: 16-byte loads (chw a multiple of 4, 16-byte aligned pointers); V = 1: the same elements one by one.  Both run the same
// arithmetic on the same lane, so they agree bit for bit.  A wave's 64 lane sums are folded by the tree v[j] += v[j + off],
// off = 32 .. 1, across the lanes (no LDS) and lane 0 stores the chunk's sums: no floating-point atomics, and nothing of the launch
// geometry in the order.  No matrix instruction: the order in which a double MFMA adds its products is not specified, so it could
// not be held to the restatement.  Contraction is off for the whole unit; sums and products go through the *_rn64 helpers.
#include "midd_internal.h"
#include "pointwise_common.h"

#pragma clang fp contract(off)

namespace midd {

constexpr int MODES_LANES = 64;                                       // a workgroup of the Gram kernels is one wave
constexpr int MODES_ROUNDS = 16;
constexpr int MODES_ROUND = 4 * MODES_LANES;                          // 256 elements a round, four per lane
constexpr int MODES_CHUNK = MODES_ROUND * MODES_ROUNDS;               // 4096: the unit of the summation order (include/midd.h)
static_assert(MODES_CHUNK == 4096, "THE ENSEMBLE MODES: chunks of 4096 elements, 16 rounds of four per lane");
constexpr int MODES_BLOCK = 8;                                        // members per block of the pair kernel
constexpr unsigned MODES_MAX_GROUPS = 16384;                          // workgroups of a Gram launch, about: more chunks than that are walked in turns
constexpr int MODES_THREADS = 256;                                    // the element-wise kernels

__device__ __forceinline__ bool modes_finite(float x) { return (__float_as_uint(x) & 0x7F800000u) != 0x7F800000u; }
__device__ __forceinline__ double modes_qnan64() { return __longlong_as_double(0x7FF8000000000000ll); }

// The member count again, as a value the compiler cannot trace back to the kernel argument.  The 64 guards and packed indices of
// a chunk's stores are uniform and do not depend on the chunk: left alone they are hoisted out of the chunk loop and held across it,
// which spills scalar registers by the hundred.  Taken anew in front of the stores they live for the stores only.
__device__ __forceinline__ int uniform_again(int K) {
    asm volatile("" : "+s"(K));
    return K;
}

// the packed index of G[i][j], i <= j < K: row i of the upper triangle starts after K + (K-1) + .. + (K-i+1) entries
__host__ __device__ __forceinline__ int gram_index(int i, int j, int K) { return i * K - i * (i - 1) / 2 + (j - i); }

// the 64 lane sums of each of N accumulators: v[j] += v[j + off] for j < off, off = 32 .. 1 (the lanes at and above off compute
// sums nobody reads)
template <int N>
__device__ __forceinline__ void fold_lanes(double (&acc)[N]) {
#pragma unroll
    for (int off = MODES_LANES / 2; off > 0; off >>= 1) {
#pragma unroll
        for (int t = 0; t < N; ++t) acc[t] = add_rn64(acc[t], __shfl_down(acc[t], (unsigned)off, MODES_LANES));
    }
}

// grid (workgroups per image, B); part [B][chunks][K (K + 1) / 2] <- the packed upper triangle of every chunk
template <int KP, int V>
__global__ __launch_bounds__(MODES_LANES)
void ensemble_gram_small_kernel(const float* __restrict__ samples, int K, unsigned long long chw, unsigned chunks,
                                double* __restrict__ part, unsigned long long* __restrict__ invalid) {
    constexpr int NP = KP * (KP + 1) / 2;
    const int lane = threadIdx.x;
    const size_t b = blockIdx.y;
    const float* src = samples + b * (size_t)K * chw;
    const int np = K * (K + 1) / 2;
    unsigned ninv = 0;
    for (unsigned chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        double acc[NP];
#pragma unroll
        for (int t = 0; t < NP; ++t) acc[t] = 0.0;
        // one element: the member-order mean, the centred members (all zero where the element is absent or invalid: their products
        // are zeros, and a sum that started at +0.0 is not changed by one), the products in the order i, then j >= i
        auto element = [&](const float (&x)[KP], bool present) {
            bool finite = true;
            double s = 0.0;
#pragma unroll
            for (int m = 0; m < KP; ++m)
                if (m < K) { finite = finite && modes_finite(x[m]); s = add_rn64(s, (double)x[m]); }
            const double mean64 = __ddiv_rn(s, (double)K);
            const bool valid = present && finite;
            ninv += (present && !finite) ? 1u : 0u;
            double d[KP];
#pragma unroll
            for (int m = 0; m < KP; ++m) d[m] = (valid && m < K) ? sub_rn64((double)x[m], mean64) : 0.0;
            int t = 0;
#pragma unroll
            for (int i = 0; i < KP; ++i) {
#pragma unroll
                for (int j = i; j < KP; ++j, ++t) acc[t] = add_rn64(acc[t], mul_rn64(d[i], d[j]));
            }
        };
        for (int r = 0; r < MODES_ROUNDS; ++r) {
            const unsigned long long e0 = (unsigned long long)chunk * MODES_CHUNK + (unsigned)(r * MODES_ROUND + 4 * lane);
            if constexpr (V == 4) {
                const bool present = e0 < chw;                  // (chw % 4 == 0: all four or none)
                f32x4 xv[KP];
#pragma unroll
                for (int m = 0; m < KP; ++m) {
                    xv[m] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
                    if (m < K && present) xv[m] = *reinterpret_cast<const f32x4*>(src + (size_t)m * chw + e0);
                }
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    float x[KP];
#pragma unroll
                    for (int m = 0; m < KP; ++m) x[m] = xv[m][p];
                    element(x, present);
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const unsigned long long e = e0 + (unsigned)p;
                    const bool present = e < chw;
                    float x[KP];
#pragma unroll
                    for (int m = 0; m < KP; ++m) x[m] = (m < K && present) ? src[(size_t)m * chw + e] : 0.0f;
                    element(x, present);
                }
            }
        }
        fold_lanes<NP>(acc);
        if (lane == 0) {
            double* dst = part + (b * chunks + chunk) * (size_t)np;
            const int Ks = uniform_again(K);
#pragma unroll
            for (int i = 0; i < KP; ++i) {
#pragma unroll
                for (int j = i; j < KP; ++j)
                    if (j < Ks) dst[gram_index(i, j, Ks)] = acc[gram_index(i, j, KP)];
            }
        }
    }
    if (ninv) atomicAdd(&invalid[b], (unsigned long long)ninv);
}

// grid (workgroups per image, B); mean [B][chw] <- the double mean of the element, or the quiet NaN where a member is not finite
template <int V>
__global__ __launch_bounds__(MODES_THREADS)
void ensemble_mean64_kernel(const float* __restrict__ samples, int K, unsigned long long chw, double* __restrict__ mean,
                            unsigned long long* __restrict__ invalid) {
    const size_t b = blockIdx.y;
    const float* src = samples + b * (size_t)K * chw;
    double* dst = mean + b * chw;
    const unsigned long long stride = (unsigned long long)gridDim.x * MODES_THREADS * V;
    unsigned ninv = 0;
    for (unsigned long long e0 = ((unsigned long long)blockIdx.x * MODES_THREADS + threadIdx.x) * V; e0 < chw; e0 += stride) {
        double s[V];
        bool finite[V];
#pragma unroll
        for (int p = 0; p < V; ++p) { s[p] = 0.0; finite[p] = true; }
#pragma unroll 4
        for (int m = 0; m < K; ++m) {
            float x[V];
            if constexpr (V == 4) {
                const f32x4 xv = *reinterpret_cast<const f32x4*>(src + (size_t)m * chw + e0);
                x[0] = xv.x; x[1] = xv.y; x[2] = xv.z; x[3] = xv.w;
            } else {
                x[0] = src[(size_t)m * chw + e0];
            }
#pragma unroll
            for (int p = 0; p < V; ++p) { finite[p] = finite[p] && modes_finite(x[p]); s[p] = add_rn64(s[p], (double)x[p]); }
        }
#pragma unroll
        for (int p = 0; p < V; ++p) {
            dst[e0 + p] = finite[p] ? __ddiv_rn(s[p], (double)K) : modes_qnan64();
            ninv += finite[p] ? 0u : 1u;
        }
    }
    if (ninv) atomicAdd(&invalid[b], (unsigned long long)ninv);
}

// grid (workgroups per image, block pairs, B); the pair p = blockIdx.y counts (bi, bj), bi <= bj < nb, row by row
template <int V>
__global__ __launch_bounds__(MODES_LANES)
void ensemble_gram_pair_kernel(const float* __restrict__ samples, const double* __restrict__ mean, int K, unsigned long long chw, unsigned chunks,
                               int nb, double* __restrict__ part) {
    constexpr int NB = MODES_BLOCK;
    const int lane = threadIdx.x;
    const size_t b = blockIdx.z;
    int bi = 0, rest = blockIdx.y;
    while (rest >= nb - bi) { rest -= nb - bi; ++bi; }
    const int bj = bi + rest;
    const int a0 = bi * NB, b0 = bj * NB;
    const bool diagonal = bi == bj;
    const float* src = samples + b * (size_t)K * chw;
    const double* mu = mean + b * chw;
    const int np = K * (K + 1) / 2;
    // The loads carry no condition: a member past K is member K - 1 read again and an absent element is element 0, both always there;
    // what they bring is dropped where the centred value is chosen.  (Sixteen guarded loads a round were sixteen exec-mask regions.)
    const float* pa[NB];
    const float* pb[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        pa[i] = src + (size_t)(a0 + i < K ? a0 + i : K - 1) * chw;
        pb[i] = src + (size_t)(b0 + i < K ? b0 + i : K - 1) * chw;
    }
    for (unsigned chunk = blockIdx.x; chunk < chunks; chunk += gridDim.x) {
        double acc[NB * NB];
#pragma unroll
        for (int t = 0; t < NB * NB; ++t) acc[t] = 0.0;
        // one element: the centred members of the two blocks (all zero where the element is absent or invalid, or the member past K:
        // their products are zeros, and a sum that started at +0.0 is not changed by one), the 64 products row by row
        auto element = [&](const float (&xa)[NB], const float (&xb)[NB], double mean64, bool present) {
            const bool valid = present && mean64 == mean64;
            double da[NB], db[NB];
#pragma unroll
            for (int i = 0; i < NB; ++i) {
                da[i] = (valid && a0 + i < K) ? sub_rn64((double)xa[i], mean64) : 0.0;
                db[i] = (valid && b0 + i < K) ? sub_rn64((double)xb[i], mean64) : 0.0;
            }
#pragma unroll
            for (int i = 0; i < NB; ++i) {
#pragma unroll
                for (int j = 0; j < NB; ++j) acc[i * NB + j] = add_rn64(acc[i * NB + j], mul_rn64(da[i], db[j]));
            }
        };
#pragma unroll 1
        for (int r = 0; r < MODES_ROUNDS; ++r) {
            const unsigned long long e0 = (unsigned long long)chunk * MODES_CHUNK + (unsigned)(r * MODES_ROUND + 4 * lane);
            if constexpr (V == 4) {
                const bool present = e0 < chw;                  // (chw % 4 == 0: all four or none)
                const unsigned long long es = present ? e0 : 0ull;
                f32x4 va[NB], vb[NB];
                double m4[4];
#pragma unroll
                for (int p = 0; p < 4; ++p) m4[p] = mu[es + p];
#pragma unroll
                for (int i = 0; i < NB; ++i) va[i] = *reinterpret_cast<const f32x4*>(pa[i] + es);
#pragma unroll
                for (int i = 0; i < NB; ++i) vb[i] = diagonal ? va[i] : *reinterpret_cast<const f32x4*>(pb[i] + es);
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    float xa[NB], xb[NB];
#pragma unroll
                    for (int i = 0; i < NB; ++i) { xa[i] = va[i][p]; xb[i] = vb[i][p]; }
                    element(xa, xb, m4[p], present);
                }
            } else {
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    const unsigned long long e = e0 + (unsigned)p;
                    const bool present = e < chw;
                    const unsigned long long es = present ? e : 0ull;
                    float xa[NB], xb[NB];
                    const double mean64 = mu[es];
#pragma unroll
                    for (int i = 0; i < NB; ++i) { xa[i] = pa[i][es]; xb[i] = diagonal ? xa[i] : pb[i][es]; }
                    element(xa, xb, mean64, present);
                }
            }
        }
        fold_lanes<NB * NB>(acc);
        if (lane == 0) {
            double* dst = part + (b * chunks + chunk) * (size_t)np;
            const int Ks = uniform_again(K);
#pragma unroll
            for (int i = 0; i < NB; ++i) {
#pragma unroll
                for (int j = 0; j < NB; ++j) {
                    const int gi = a0 + i, gj = b0 + j;
                    if (gi <= gj && gj < Ks) dst[gram_index(gi, gj, Ks)] = acc[i * NB + j];
                }
            }
        }
    }
}

// one thread per (image, i, j): the chunk sums of G[min(i, j)][max(i, j)] one by one from 0 in chunk order.  The loads of a batch do
// not depend on each other, the adds do
constexpr int MODES_FINAL_BATCH = 16;
__global__ __launch_bounds__(MODES_THREADS)
void ensemble_gram_final_kernel(const double* __restrict__ part, int B, int K, unsigned chunks, double* __restrict__ gram) {
    const unsigned t = blockIdx.x * MODES_THREADS + threadIdx.x;
    const unsigned kk = (unsigned)(K * K);
    if (t >= (unsigned)B * kk) return;
    const unsigned b = t / kk, i = (t % kk) / (unsigned)K, j = t % (unsigned)K;
    const size_t np = (size_t)(K * (K + 1) / 2);
    const double* p = part + (size_t)b * chunks * np + gram_index((int)(i < j ? i : j), (int)(i < j ? j : i), K);
    double s = 0.0;
    unsigned c = 0;
    for (; c + MODES_FINAL_BATCH <= chunks; c += MODES_FINAL_BATCH) {
        double v[MODES_FINAL_BATCH];
#pragma unroll
        for (int q = 0; q < MODES_FINAL_BATCH; ++q) v[q] = p[(size_t)(c + q) * np];
#pragma unroll
        for (int q = 0; q < MODES_FINAL_BATCH; ++q) s = add_rn64(s, v[q]);
    }
    for (; c < chunks; ++c) s = add_rn64(s, p[(size_t)c * np]);
    gram[t] = s;
}

// grid (workgroups per image, B); out [B][M][chw] <- (float)(sum_k w[b][j][k] * d_k), the quiet NaN where a member is not finite
template <int MP, int V>
__global__ __launch_bounds__(MODES_THREADS)
void ensemble_project_kernel(const float* __restrict__ samples, int K, unsigned long long chw, const double* __restrict__ weights, int M,
                             float* __restrict__ out) {
    const size_t b = blockIdx.y;
    const float* src = samples + b * (size_t)K * chw;
    const double* w = weights + b * (size_t)M * K;
    float* dst = out + b * (size_t)M * chw;
    const unsigned long long stride = (unsigned long long)gridDim.x * MODES_THREADS * V;
    auto load = [&](int m, unsigned long long e0, float (&x)[V]) {
        if constexpr (V == 4) {
            const f32x4 xv = *reinterpret_cast<const f32x4*>(src + (size_t)m * chw + e0);
            x[0] = xv.x; x[1] = xv.y; x[2] = xv.z; x[3] = xv.w;
        } else {
            x[0] = src[(size_t)m * chw + e0];
        }
    };
    for (unsigned long long e0 = ((unsigned long long)blockIdx.x * MODES_THREADS + threadIdx.x) * V; e0 < chw; e0 += stride) {
        double s[V], mean64[V], acc[MP][V];
        bool finite[V];
#pragma unroll
        for (int p = 0; p < V; ++p) { s[p] = 0.0; finite[p] = true; }
#pragma unroll 4
        for (int m = 0; m < K; ++m) {
            float x[V];
            load(m, e0, x);
#pragma unroll
            for (int p = 0; p < V; ++p) { finite[p] = finite[p] && modes_finite(x[p]); s[p] = add_rn64(s[p], (double)x[p]); }
        }
#pragma unroll
        for (int p = 0; p < V; ++p) {
            mean64[p] = __ddiv_rn(s[p], (double)K);
#pragma unroll
            for (int j = 0; j < MP; ++j) acc[j][p] = 0.0;
        }
#pragma unroll 2
        for (int m = 0; m < K; ++m) {
            float x[V];
            load(m, e0, x);
#pragma unroll
            for (int p = 0; p < V; ++p) {
                const double d = sub_rn64((double)x[p], mean64[p]);
#pragma unroll
                for (int j = 0; j < MP; ++j)
                    if (j < M) acc[j][p] = add_rn64(acc[j][p], mul_rn64(w[j * K + m], d));
            }
        }
        const float qnan = __uint_as_float(0x7FC00000u);
#pragma unroll
        for (int j = 0; j < MP; ++j)
            if (j < M) {
                if constexpr (V == 4) {
                    f32x4 o;
#pragma unroll
                    for (int p = 0; p < 4; ++p) o[p] = finite[p] ? __double2float_rn(acc[j][p]) : qnan;
                    *reinterpret_cast<f32x4*>(dst + (size_t)j * chw + e0) = o;
                } else {
                    dst[(size_t)j * chw + e0] = finite[0] ? __double2float_rn(acc[j][0]) : qnan;
                }
            }
    }
}

// ---------------------------------------------------------------------------------------------------------------- launches
unsigned long long ensemble_gram_chunks(unsigned long long chw) { return (chw + MODES_CHUNK - 1) / MODES_CHUNK; }

// the chunk sums, double [B][chunks][K (K + 1) / 2], then for K > 8 the means, double [B][chw]
size_t ensemble_gram_workspace_bytes(int B, int K, unsigned long long chw) {
    const size_t part = (size_t)B * ensemble_gram_chunks(chw) * (size_t)(K * (K + 1) / 2);
    return (part + (K > MODES_BLOCK ? (size_t)B * chw : 0)) * sizeof(double);
}

// workgroups of an element-wise launch: one element group a thread, at most MODES_MAX_GROUPS over the batch
static unsigned elementwise_groups(int B, unsigned long long chw, int V) {
    const unsigned long long want = (chw / V + MODES_THREADS - 1) / MODES_THREADS;
    const unsigned cap = MODES_MAX_GROUPS / (unsigned)B ? MODES_MAX_GROUPS / (unsigned)B : 1u;
    return (unsigned)(want < cap ? (want ? want : 1) : cap);
}

template <int KP>
static void gram_small_dispatch(const float* samples, int B, int K, unsigned long long chw, unsigned chunks, unsigned gx, bool v4,
                                double* part, unsigned long long* invalid, hipStream_t s) {
    if (v4) hipLaunchKernelGGL((ensemble_gram_small_kernel<KP, 4>), dim3(gx, B), dim3(MODES_LANES), 0, s, samples, K, chw, chunks, part, invalid);
    else hipLaunchKernelGGL((ensemble_gram_small_kernel<KP, 1>), dim3(gx, B), dim3(MODES_LANES), 0, s, samples, K, chw, chunks, part, invalid);
}

hipError_t ensemble_gram_launch(const float* samples, int B, int K, unsigned long long chw, double* gram, unsigned long long* invalid,
                                double* ws, hipStream_t s) {
    if (B < 1 || B > 65535 || K < 2 || K > MODES_MAX_MEMBERS || chw < 1 || chw >= (1ull << 32) || !samples || !gram || !invalid || !ws)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetAsync(invalid, 0, (size_t)B * sizeof(unsigned long long), s);
    if (e != hipSuccess) return e;
    const unsigned chunks = (unsigned)ensemble_gram_chunks(chw);
    const int nb = (K + MODES_BLOCK - 1) / MODES_BLOCK, pairs = K > MODES_BLOCK ? nb * (nb + 1) / 2 : 1;
    // every workgroup of an (image, pair) walks the same number of chunks (the last one may walk fewer)
    const unsigned cap = MODES_MAX_GROUPS / (unsigned)(B * pairs) ? MODES_MAX_GROUPS / (unsigned)(B * pairs) : 1u;
    const unsigned turns = (chunks + cap - 1) / cap;
    const unsigned gx = (chunks + turns - 1) / turns;
    const bool v4 = chw % 4 == 0 && aligned16(samples);
    double* part = ws;
    if (K <= 2) gram_small_dispatch<2>(samples, B, K, chw, chunks, gx, v4, part, invalid, s);
    else if (K <= 4) gram_small_dispatch<4>(samples, B, K, chw, chunks, gx, v4, part, invalid, s);
    else if (K <= MODES_BLOCK) gram_small_dispatch<8>(samples, B, K, chw, chunks, gx, v4, part, invalid, s);
    else {
        double* mean = ws + (size_t)B * chunks * (size_t)(K * (K + 1) / 2);
        const dim3 mgrid(elementwise_groups(B, chw, v4 ? 4 : 1), B);
        if (v4) hipLaunchKernelGGL((ensemble_mean64_kernel<4>), mgrid, dim3(MODES_THREADS), 0, s, samples, K, chw, mean, invalid);
        else hipLaunchKernelGGL((ensemble_mean64_kernel<1>), mgrid, dim3(MODES_THREADS), 0, s, samples, K, chw, mean, invalid);
        e = hipGetLastError();
        if (e != hipSuccess) return e;
        if (v4) hipLaunchKernelGGL((ensemble_gram_pair_kernel<4>), dim3(gx, pairs, B), dim3(MODES_LANES), 0, s, samples, mean, K, chw, chunks, nb, part);
        else hipLaunchKernelGGL((ensemble_gram_pair_kernel<1>), dim3(gx, pairs, B), dim3(MODES_LANES), 0, s, samples, mean, K, chw, chunks, nb, part);
    }
    e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ensemble_gram_final_kernel, dim3((B * K * K + MODES_THREADS - 1) / MODES_THREADS), dim3(MODES_THREADS), 0, s, part, B, K, chunks, gram);
    return hipGetLastError();
}

template <int MP>
static void project_dispatch(const float* samples, int B, int K, unsigned long long chw, const double* weights, int M, float* out, bool v4, hipStream_t s) {
    const dim3 grid(elementwise_groups(B, chw, v4 ? 4 : 1), B);
    if (v4) hipLaunchKernelGGL((ensemble_project_kernel<MP, 4>), grid, dim3(MODES_THREADS), 0, s, samples, K, chw, weights, M, out);
    else hipLaunchKernelGGL((ensemble_project_kernel<MP, 1>), grid, dim3(MODES_THREADS), 0, s, samples, K, chw, weights, M, out);
}

hipError_t ensemble_project_launch(const float* samples, int B, int K, unsigned long long chw, const double* weights, int M, float* out, hipStream_t s) {
    if (B < 1 || B > 65535 || K < 2 || K > MODES_MAX_MEMBERS || chw < 1 || chw >= (1ull << 32) || M < 1 || M > MODES_MAX_MODES || !samples || !weights || !out)
        return hipErrorInvalidValue;
    const bool v4 = chw % 4 == 0 && aligned16(samples) && aligned16(out);
    if (M <= 1) project_dispatch<1>(samples, B, K, chw, weights, M, out, v4, s);
    else if (M <= 2) project_dispatch<2>(samples, B, K, chw, weights, M, out, v4, s);
    else if (M <= 4) project_dispatch<4>(samples, B, K, chw, weights, M, out, v4, s);
    else project_dispatch<8>(samples, B, K, chw, weights, M, out, v4, s);
    return hipGetLastError();
}

}  // namespace midd
