// What more than one of the pointwise translation units needs (in_conv.hip, out_conv.hip, ensemble.hip, tiles.hip, dihedral.hip,
// resample.hip): the 16-byte vector type, the alignment test of the V = 4 paths, the GroupNorm totals of a pointwise producer,
// and the double-precision operations that are rounded on their own.
#pragma once
#include "midd_internal.h"

namespace midd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

// ------------------------------------------------------------------------------ statistics of a pointwise producer
// The HBM-bound producers (in_conv.hip, resample.hip) also leave the GroupNorm totals of their output (stats_common.h) -- round 1/2 read the
// tensor a second time for that (chan_total_kernel: 4 launches per forward).  A workgroup owns a pixel range of ONE sample;
// thread = (pixel lane pl < ppi, channel group); each thread sums ITS NV channels over the pixels it walks (fp32, fixed
// order), the lanes are folded per channel in fp64 in lane order, rounded once to fp32, and published with exact integer
// atomics.  scratch: 2 * C * ppi floats of LDS; acc: (C + 2) * 6 words.
template <int NV>
__device__ __forceinline__ void pointwise_publish(const float (&sum)[NV], const float (&sq)[NV], bool active, int pl, int ppi, int cgrp,
                                                  int C, float* scratch, stat_word* acc, stat_word* tot, int b, int bs, int rep,
                                                  int replica, int tid, int nthreads = 256, int c0 = 0, int ncol = -1) {
    if (ncol < 0) ncol = C;                       // the workgroup's channels: [c0, c0 + ncol) of the tensor's C; cgrp counts inside them
    if (active) {
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            scratch[(size_t)(cgrp * NV + e) * ppi + pl] = sum[e];
            scratch[(size_t)(ncol + cgrp * NV + e) * ppi + pl] = sq[e];
        }
    }
    auto fold = [&](int i) {
        double t = 0;
        for (int l = 0; l < ppi; ++l) t += (double)scratch[(size_t)i * ppi + l];
        return (float)t;
    };
    stat_publish(tot, b, C, bs, rep, replica, c0, ncol, fold, acc, tid, nthreads);
}

// pixels a workgroup of 256 threads walks: ~4 per pixel lane, at most 1024 workgroups per sample
static inline int pointwise_rows(int HW, int ppi) {
    int r = (HW + ppi * 4 - 1) / (ppi * 4);
    return r < 1 ? 1 : (r > 1024 ? 1024 : r);
}

// ------------------------------------------------------------------------------ double operations rounded on their own
// Where THE ARITHMETIC IS FIXED (include/midd.h: mi_ensemble_reduce, mi_tile_blend, mi_ensemble_quantiles, mi_dihedral_reduce)
// it is in double precision, every operation rounded to nearest on its own.  hipcc's __dadd_rn / __dmul_rn are the plain operators, which -ffp-contract=fast fuses (q += d * d became one v_fmac_f64), so the
// three operations are functions of this file compiled with contraction off; division and square root are the correctly
// rounded library ones (the FMAs left in the ISA are inside those two).
__device__ __forceinline__ double add_rn64(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double sub_rn64(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double mul_rn64(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}

}  // namespace midd
