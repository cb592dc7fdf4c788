// Fused self-attention on split-fp16 MFMAs (three v_mfma_f32_16x16x32_f16 per product, fp32
// accumulate) — the f16x3 counterpart of attention_f32.hip, same transposed-score trick.
//
// Replaces AttentionBlock.forward's matmul / softmax / matmul
// (/root/reference/Backend/DDIM/DDIMModel.py:149-162; heads = 2, head_dim = C/2, q scaled by
// head_dim^-0.5, full softmax over the keys — the reference's 512-query chunking is exact; the hybrid
// copy's un-chunked form with the scale after QK^T, hybrid3diffusionspeed.py:295-301, is the same function).
//
//   S^T[key][q] = K . Q^T   A = K rows (16 B = 8 consecutive d per lane), B = Q^T from registers
//   P           = exp2(S^T - m)  online softmax; the lane that owns a query column owns its m, l
//   O^T[d][q]  += V^T . P^T  A = V^T, B = P^T straight from the score accumulators:
//                            the 32-wide k index of this MFMA is permuted so that element j of lane group kq
//                            is key 16*(j>>2)+4*kq+(j&3) of the key pair-block — the keys the lane already holds.
// Every fp32 operand x is used as x*2^s = hi + lo (fp16 each, exact power-of-two prescale):
// q,k,v: s = 4; p in [0,1]: s = 10; hi.hi + hi.lo + lo.hi reproduces the fp32 product to ~2^-21.
//
// Structure:
//   * workgroup = 4 waves x 32 queries (two 16-query MFMA column tiles per wave): every K / V fragment read
//     from LDS feeds six MFMAs;
//   * the keys are split `ksplit` ways over workgroups (flash-decoding style) so that ~256-512 workgroups exist at any
//     batch size; each split leaves (m, l, unnormalised O^T);
//   * K / V tiles of 32 keys go global -> LDS by LDS-DMA (global_load_lds_dwordx4, 1 KiB per wave
//     instruction, per-lane source addresses so the padded, conflict-free LDS rows need no padded global
//     image) into a two-stage ring: one barrier per tile, the next tile in flight under the MFMAs.
// Round 3: the attention block is THREE launches (it was five).  The qkv projection's epilogue writes q (fp32 [B][N][C]) and
// the split-fp16 K and V images this kernel stages (conv1x1_f16x3.hip, ATT_QKV_OUT) -- attention_prep_kernel is gone, and
// so is the transposed V image: V is staged [key][d] like K and its MFMA A fragments (V^T) come from ds_read_b64_tr_b16,
// the transposing LDS read (each 16-lane group reads a 4-key x 16-d block and receives it d-major).  The partials are
// ALWAYS written (also for one split) and combined by the output projection while it loads its operand
// (conv1x1_f16x3.hip, ATT_PART_IN) -- attention_combine_kernel and the normalised [B][N][C] tensor are gone.
#include "midd_internal.h"
#include <cstdlib>

namespace midd {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

constexpr int A16_KT = 32;                 // keys per LDS tile
constexpr int A16_QW = 32;                 // queries per wave
constexpr int A16_QB = 4 * A16_QW;         // queries per workgroup
constexpr int A16_MAX_SPLIT = 8;
constexpr float A16_QKV_SCALE = 16.0f;     // 2^4
constexpr float A16_P_SCALE = 1024.0f;     // 2^10
constexpr float A16_P_SHIFT = 10.0f;       // log2 of it: folded into the softmax exponent

__device__ __forceinline__ void split1(float x, _Float16& hi, _Float16& lo) {
    hi = (_Float16)x;
    lo = (_Float16)(x - (float)hi);
}

// hi = fp16(x) pairs by v_cvt_pk_f16_f32, lo = fp16(x - hi) by v_fma_mix{lo,hi}_f16 (f16x3_common.h: split_pair)
__device__ __forceinline__ void att_split_pair(float x0, float x1, unsigned& hi, unsigned& lo) {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    h2 h;
    h[0] = (_Float16)x0; h[1] = (_Float16)x1;
    hi = __builtin_bit_cast(unsigned, h);
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]" : "=v"(lo) : "v"(hi), "v"(x0));
    asm("v_fma_mixhi_f16 %0, %1, -1.0, %2 op_sel:[1,0,0] op_sel_hi:[1,0,0]" : "+v"(lo) : "v"(hi), "v"(x1));
}

template <int PL>
__device__ __forceinline__ void att_planes_pair(float x0, float x1, unsigned& hi, unsigned& lo) {
    if constexpr (PL == 2) att_split_pair(x0, x1, hi, lo);
    else {                                      // compute "f16": the fp16 rounding alone
        typedef _Float16 h2 __attribute__((ext_vector_type(2)));
        h2 h;
        h[0] = (_Float16)x0; h[1] = (_Float16)x1;
        hi = __builtin_bit_cast(unsigned, h);
        lo = 0u;
    }
}

__device__ __forceinline__ void att_dma16(const void* gsrc, char* lds_dst_wave_base) {
    __builtin_amdgcn_global_load_lds((const void __attribute__((address_space(1)))*)gsrc,
                                     (void __attribute__((address_space(3)))*)lds_dst_wave_base, 16, 0, 0);
}

// PL: fp16 planes per operand -- 2 = hi | lo (f16x3), 1 = the rounded value alone (compute "f16": attention_f16_kernel)
template <int D, int PL = 2>
struct Att16Geom {
    static constexpr int KCH = D / 8 + 2;                  // 16-byte chunks per K / V row in LDS: D halfs + 16 pad (224-B rows at D = 96:
    static constexpr int KROW = KCH * 16;                  //   conflict-free ds_read_b128 row reads AND ds_read_b64_tr_b16 block reads)
    static constexpr int KPLANE = A16_KT * KROW;           // bytes of one plane (hi or lo) of a 32-key tile
    static constexpr int STAGE = 2 * PL * KPLANE;          // K hi | K lo | V hi | V lo  (one plane: K | V)
    static constexpr int CHUNKS = 2 * PL * A16_KT * KCH;
    static constexpr int PIECES = CHUNKS / 64;             // 1 KiB DMA pieces per stage (= PL KCH)
    static constexpr int PPW = (PIECES + 3) / 4;           // per wave
    static_assert(CHUNKS % 64 == 0, "whole DMA pieces");
};

// The kernel, compiled twice from one text: two planes / three products, one plane / one product
#define MIDD_ATT16_KERNEL attention_f16x3_kernel
#define MIDD_ATT16_PL 2
#include "attention_f16x3_body.h"
#undef MIDD_ATT16_KERNEL
#undef MIDD_ATT16_PL
#define MIDD_ATT16_KERNEL attention_f16_kernel
#define MIDD_ATT16_PL 1
#include "attention_f16x3_body.h"
#undef MIDD_ATT16_KERNEL
#undef MIDD_ATT16_PL

static int att16_npad(int N) { return ((N + 63) / 64) * 64; }

Att16Layout attention16_layout(int B, int N, int C, int planes) {
    Att16Layout L{};
    L.npad = att16_npad(N);
    const size_t kbytes = (((size_t)B * planes * L.npad * C * sizeof(_Float16)) + 255) & ~(size_t)255;  // K (and V): [B][heads][planes][Npad][D], C = heads * D
    const size_t pobytes = (((size_t)A16_MAX_SPLIT * B * N * C * sizeof(float)) + 255) & ~(size_t)255;
    const size_t mlbytes = (((size_t)A16_MAX_SPLIT * B * 2 * N * 2 * sizeof(float)) + 255) & ~(size_t)255;   // 2 heads x (m, l)
    L.k_off = 0; L.v_off = kbytes; L.po_off = 2 * kbytes; L.ml_off = L.po_off + pobytes; L.bytes = L.ml_off + mlbytes;
    return L;
}

// Key split (flash-decoding) for occupancy: up to two workgroups per CU (what the LDS allows) while a split keeps
// >= 16 tiles of 32 keys (N = 4096: 375 -> 326 us per attention block), then up to one per CU down to two tiles per
// split (a 512 target with short splits measured slower at N = 1024).  The doubling loops only give a target: the
// split count is then SHRUNK to the splits that own at least one tile (ceil(tiles / tiles_per_split)) -- e.g.
// N = 784 (224x224 / 8): 25 tiles, target 8 -> 4 tiles per split -> 7 splits (round 2 returned an error there).
void attention16_split(int N, int heads, int split_B, int* ksplit_out, int* tiles_per_split) {
    const int qblocks = (N + A16_QB - 1) / A16_QB, tiles = (N + A16_KT - 1) / A16_KT;
    int ksplit = 1;
    while ((long)qblocks * heads * split_B * ksplit < 512 && ksplit * 2 <= A16_MAX_SPLIT && tiles / (ksplit * 2) >= 16) ksplit *= 2;
    while ((long)qblocks * heads * split_B * ksplit < 256 && ksplit * 2 <= A16_MAX_SPLIT && tiles / (ksplit * 2) >= 2) ksplit *= 2;
    const int tps = (tiles + ksplit - 1) / ksplit;
    ksplit = (tiles + tps - 1) / tps;               // every split owns >= 1 tile, and every tile starts below N
    *ksplit_out = ksplit; *tiles_per_split = tps;
}

hipError_t attention16_launch(const float* q, const _Float16* Kp, const _Float16* Vp, float* part_o, float* part_ml,
                              int B, int ksplit, int tps, int N, int C, int heads, hipStream_t s, int planes) {
    const int D = C / heads;
    if (planes != 1 && planes != 2) return hipErrorInvalidValue;
    if (C % heads || !attention_supported(D) || D % 32 || heads != 2) return hipErrorInvalidValue;
    const int tiles = (N + A16_KT - 1) / A16_KT;
    if (ksplit < 1 || ksplit > A16_MAX_SPLIT || tps < 1 || (long)(ksplit - 1) * tps >= tiles || (long)ksplit * tps < tiles) return hipErrorInvalidValue;
    const float qscale = (float)((1.0 / sqrt((double)D)) * 1.4426950408889634);
    const int Npad = att16_npad(N);
    const int qblocks = (N + A16_QB - 1) / A16_QB;
    hipError_t e = hipSuccess;
#define MIDD_ATT_K(DD, KERNEL, PL)                                                                                          \
    {                                                                                                                       \
        constexpr int lds_bytes = 2 * Att16Geom<DD, PL>::STAGE;                                                             \
        static int raised[MIDD_MAX_DEVICES] = {};                                                                           \
        e = ensure_dynamic_lds(reinterpret_cast<const void*>(&KERNEL<DD>), lds_bytes, raised);                              \
        if (e != hipSuccess) return e;                                                                                      \
        hipLaunchKernelGGL((KERNEL<DD>), dim3(qblocks * ksplit, heads, B), dim3(256), lds_bytes, s,                         \
                           q, Kp, Vp, part_o, part_ml, N, Npad, C, qscale, ksplit, tps);                                    \
    }
#define MIDD_ATT(DD) if (planes == 2) MIDD_ATT_K(DD, attention_f16x3_kernel, 2) else MIDD_ATT_K(DD, attention_f16_kernel, 1)
    switch (D) {
        case 32:  MIDD_ATT(32) break;
        case 64:  MIDD_ATT(64) break;
        case 96:  MIDD_ATT(96) break;
        case 128: MIDD_ATT(128) break;
    }
#undef MIDD_ATT
#undef MIDD_ATT_K
    return hipGetLastError();
}

}  // namespace midd
