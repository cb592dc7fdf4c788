// Order statistics of a pixel's ensemble members in registers (include/midd.h: mi_ensemble_quantiles; ensemble.hip:
// ensemble_quantiles_kernel, tiles.hip: tile_blend_quantiles_kernel, dihedral.hip: dihedral_quantiles_kernel); tests/quantile_reference.py restates it in numpy.
//   key:      k = bits ^ (sign ? 0xFFFFFFFF : 0x80000000) -- an unsigned integer whose order is the total order
//             -inf < ... < -0.0 < +0.0 < ... < +inf of the floats, so a compare-exchange is one unsigned min and one unsigned max:
//             no NaN case, no signed-zero case; equal keys are equal bits, so the sorted sequence is unique
//   network:  Batcher's odd-even merge sort for N = 2^j keys (1, 5, 19, 63, 191, 543 compare-exchanges for N = 2 .. 64), generated
//             at compile time; every compare-exchange names its two registers as template arguments, so the key array is never
//             indexed by a run-time value and stays in registers.  A member count K < N is padded with the key 0xFFFFFFFF, which
//             sorts behind +inf: the K real keys end in k[0 .. K-1]
//   pick:     k[i] for a run-time i as a chain of selects over the constant indices -- again no run-time register index
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "pointwise_common.h"

namespace midd {

constexpr uint32_t ORDER_KEY_PAD = 0xFFFFFFFFu;

__host__ __device__ __forceinline__ uint32_t order_key(uint32_t bits) {
    return bits ^ ((bits >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__host__ __device__ __forceinline__ uint32_t order_bits(uint32_t key) {
    return key ^ ((key >> 31) ? 0x80000000u : 0xFFFFFFFFu);
}

template <int N>
struct SortNet {
    static_assert(N >= 2 && (N & (N - 1)) == 0, "a power of two");
    int a[N * 9], b[N * 9];               // compare-exchange i orders (k[a[i]], k[b[i]]), a[i] < b[i]; N * 9 >= their number up to N = 64
    int n;
};

template <int N>
constexpr SortNet<N> make_sort_net() {
    SortNet<N> s{};
    for (int p = 1; p < N; p *= 2)
        for (int k = p; k >= 1; k /= 2)
            for (int j = k % p; j <= N - 1 - k; j += 2 * k)
                for (int i = 0; i < k && i <= N - j - k - 1; ++i)
                    if ((i + j) / (2 * p) == (i + j + k) / (2 * p)) {
                        s.a[s.n] = i + j;
                        s.b[s.n] = i + j + k;
                        ++s.n;
                    }
    return s;
}

template <int N>
struct SortNetOf { static constexpr SortNet<N> net = make_sort_net<N>(); };

// compare-exchanges [LO, HI) of the network, in order
template <int N, int LO, int HI>
__host__ __device__ __forceinline__ void sort_net_apply(uint32_t (&k)[N]) {
    if constexpr (HI - LO == 1) {
        constexpr int A = SortNetOf<N>::net.a[LO], B = SortNetOf<N>::net.b[LO];
        static_assert(0 <= A && A < B && B < N, "register indices");
        const uint32_t lo = k[A] < k[B] ? k[A] : k[B], hi = k[A] < k[B] ? k[B] : k[A];
        k[A] = lo;
        k[B] = hi;
    } else if constexpr (HI - LO > 1) {
        sort_net_apply<N, LO, LO + (HI - LO) / 2>(k);
        sort_net_apply<N, LO + (HI - LO) / 2, HI>(k);
    }
}

template <int N>
__host__ __device__ __forceinline__ void sort_keys(uint32_t (&k)[N]) {
    static_assert(SortNetOf<N>::net.n <= N * 9, "network size");
    sort_net_apply<N, 0, SortNetOf<N>::net.n>(k);
}

// (template recursion, not a loop: a rolled `r = (j == i) ? k[j] : r` loop is folded back into the indexed load k[i], and an array
// indexed by a run-time value lives in scratch)
template <int N, int J>
__host__ __device__ __forceinline__ uint32_t pick_key_from(const uint32_t (&k)[N], int i, uint32_t r) {
    if constexpr (J < N) return pick_key_from<N, J + 1>(k, i, (J == i) ? k[J] : r);
    else return r;
}

template <int N>
__host__ __device__ __forceinline__ uint32_t pick_key(const uint32_t (&k)[N], int i) {
    return pick_key_from<N, 1>(k, i, k[0]);
}

// the interpolation between two order statistics, every operation rounded on its own (pointwise_common.h), and the level rules
struct QuantilePos { int lo, hi; double g; };

__device__ __forceinline__ QuantilePos quantile_pos(double q, int K) {
    const double pos = mul_rn64(q, (double)(K - 1));
    QuantilePos p;
    p.lo = (int)floor(pos);
    p.hi = min(p.lo + 1, K - 1);
    p.g = sub_rn64(pos, (double)p.lo);
    return p;
}

template <int KP>
__device__ __forceinline__ float quantile_of_sorted(const uint32_t (&key)[KP], const QuantilePos& p, int K, bool has_nan) {
    const float s_lo = __uint_as_float(order_bits(pick_key(key, p.lo)));
    const float s_hi = __uint_as_float(order_bits(pick_key(key, p.hi)));
    const float r = __double2float_rn(add_rn64((double)s_lo, mul_rn64(p.g, sub_rn64((double)s_hi, (double)s_lo))));
    const float v = (K == 1) ? s_lo : r;                    // one member: every quantile is that member, bit for bit
    return (has_nan || v != v) ? __uint_as_float(0x7FC00000u) : v;
}

__device__ __forceinline__ bool is_nan_bits(uint32_t bits) { return (bits & 0x7FFFFFFFu) > 0x7F800000u; }

static inline bool quantile_levels_ok(const QuantileLevels& ql) {
    if (ql.nq < 1 || ql.nq > QUANTILE_MAX_LEVELS) return false;
    for (int i = 0; i < ql.nq; ++i)
        if (!(ql.q[i] >= 0.0 && ql.q[i] <= 1.0)) return false;
    return true;
}

}  // namespace midd
