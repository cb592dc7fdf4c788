// 1x1 convolution (res_conv, attention qkv / proj: DDIMModel.py:52,90-91 / cddpmModels.py:55,104-105) in
// f16x3 arithmetic (see conv_mfma_f16x3.hip for the number format), as a GEMM  out[p][co] = sum_ci act(x[p][ci]) * W[co][ci]
// over the flattened pixels of a sample.
//
// A 1x1 conv has no halo and no taps, so the general kernel's machinery (raw staging in LDS, transform pass,
// chunk barriers, weight ring) is pure latency here: with one K-step per chunk it serialises a DMA round trip
// per 32 channels.  This kernel instead
//   * loads each lane's B operand straight from global memory: lane (pixel p16, k-quarter kq) of a 16x16x32
//     MFMA needs channels kq*8 .. kq*8+7 of its pixel = 32 contiguous bytes inside one 16-channel block of the channel-blocked
//     layout (midd_internal.h; 16 pixel lanes x two k-quarters read one contiguous KiB); GroupNorm-apply / SiLU /
//     2^s prescale / hi-lo split happen in registers (each element once per workgroup, as before);
//   * keeps ALL weights of the workgroup's 16*NT output channels in LDS (Cin * NT * 64 B: 36 KB at Cin = 192),
//     fetched once by LDS-DMA and reused for every pixel tile the persistent workgroup walks;
//   * has no barrier in the K loop; the activation loads run two K-steps ahead in registers, across tile borders.
// Epilogue and contract are those of conv_mfma_f16x3.hip (bias / time embedding / residual, GroupNorm partial
// sums of the output per (workgroup, wave) row).  Weight pack: pack_conv_f16x3 (midd_weights.hip), 32 channels per step.
//
// Attention hand-off (round 3: the attention block is three launches, qkv -> attention -> proj; it was five):
//   ATT_QKV_OUT  the qkv projection writes what the attention kernel stages instead of an fp32 [B][N][3C] tensor that a
//                separate pass re-read and converted: q as fp32 [B][N][C], k and v as split-fp16 images
//                [B][heads][hi|lo][Npad][D] (x 2^4; rows of keys >= N zeroed).  |k|, |v| >= 4094 cannot be represented:
//                the status word gets MI_STATUS_FP16_RANGE (mi_status) instead of a silent inf;
//   ATT_PART_IN  the output projection reads the attention kernel's key-split partials (m_s, l_s, O_s) directly: the splits
//                are extra K steps over the same weights, and each loaded element is scaled by
//                2^(m_s - M) / (L 2^14), M = max_s m_s, L = sum_s l_s 2^(m_s - M) -- the flash-decoding combine, in split
//                order, applied where the operand is converted anyway (it was a kernel of its own that wrote a tensor).
#include "f16x3_common.h"
#include <cstdlib>

namespace midd {

constexpr int C1_MAX_SPLIT = 8;                  // == A16_MAX_SPLIT (attention_f16x3.hip)

// Geometry of the (mt, nt) tile (4 waves, 256 threads), written down once as plain integers: Conv1Geom<> hands it to the kernel as
// constants, conv1x1_launch_info (which launch1 calls for its grid and LDS bytes) evaluates it at run time.
struct Conv1Tile {
    int mt, nt;
    int pl = 2;                                      // fp16 planes per operand: 2 = hi | lo (f16x3), 1 = the rounded value alone (compute "f16")
    int bm = 4 * mt * 16;                            // pixels per tile
    int wstep = nt * pl * 1024;                      // bytes of one K-step's weights (pl planes, nt cout tiles)
    int stat_floats = 4 * 2 * nt * 16, add_floats = nt * 16;
    int coef_floats = C1_MAX_SPLIT * 2 * bm;         // ATT_PART_IN: [split][head][pixel of the tile]
    constexpr int weight_bytes(int cin) const { const int w = ((cin + 31) / 32) * wstep; return w < 4096 ? 4096 : w; }      // also the statistics scratch at the end
    constexpr int lds_bytes(int cin, int att_mode) const {
        return weight_bytes(cin) + (stat_floats + add_floats) * 4 + 2 * cin * 4 + 64 + (att_mode == ATT_PART_IN ? coef_floats * 4 : 0);
    }
};
template <int MT, int NT, int PL = 2>
struct Conv1Geom {
    static constexpr Conv1Tile g{MT, NT, PL};
    static constexpr int NW = 4, NTHREADS = 256, BM = g.bm, WSTEP = g.wstep, STAT_FLOATS = g.stat_floats, ADD_FLOATS = g.add_floats;
};

// The kernel, compiled twice from one text: two planes / three products, one plane / one product
#define MIDD_CONV1_KERNEL conv1x1_f16x3_kernel
#define MIDD_CONV1_PL 2
#include "conv1x1_f16x3_body.h"
#undef MIDD_CONV1_KERNEL
#undef MIDD_CONV1_PL
#define MIDD_CONV1_KERNEL conv1x1_f16_kernel
#define MIDD_CONV1_PL 1
#include "conv1x1_f16x3_body.h"
#undef MIDD_CONV1_KERNEL
#undef MIDD_CONV1_PL

template <int MT, int NT, int ATT, int PL>
static hipError_t launch1(const ConvArgs& a0, hipStream_t s) {
    ConvArgs a = a0;
    ConvLaunchInfo li{};
    (void)conv1x1_launch_info(a.C0 + a.C1, a.Cout, a.B, a.OH, a.OW, ConvTile{1, 1, 0, MT, NT, 4, 1, 0, PL}, a.persist_wgs, ATT, &li);
    a.tiles_x = li.tiles_x; a.tiles_y = 1; a.wgs_per_img = li.wgs_per_img;
    if (li.lds_bytes > 160 * 1024) return hipErrorInvalidValue;
    {
        static int raised[MIDD_MAX_DEVICES] = {};          // per instantiation and device
        hipError_t e = ensure_dynamic_lds(PL == 2 ? reinterpret_cast<const void*>(&conv1x1_f16x3_kernel<MT, NT, ATT>)
                                                  : reinterpret_cast<const void*>(&conv1x1_f16_kernel<MT, NT, ATT>), li.lds_bytes, raised);
        if (e != hipSuccess) return e;
    }
    if constexpr (PL == 2) hipLaunchKernelGGL((conv1x1_f16x3_kernel<MT, NT, ATT>), dim3(li.grid_x, li.grid_y), dim3(256), li.lds_bytes, s, a);
    else hipLaunchKernelGGL((conv1x1_f16_kernel<MT, NT, ATT>), dim3(li.grid_x, li.grid_y), dim3(256), li.lds_bytes, s, a);
    return hipGetLastError();
}

// tile.tw == 0 marks the flattened-pixel 1x1 kernel (tile = 64*mt pixels x 16*nt couts, 4 waves)
bool conv1x1_pick_tile(int Cin, int Cout, int B, int OH, int OW, ConvTile* t) {
    if (Cout % 16 || Cin % 16) return false;
    const int nt = (Cout % 48 == 0) ? 3 : (Cout % 32 == 0) ? 2 : 1;
    const long wgs2 = (long)B * ((OH * OW + 127) / 128) * (Cout / (16 * nt));
    const int mt = wgs2 >= 512 ? 2 : 1;                      // small maps: 64-pixel tiles, twice the workgroups
    if (((Cin + 31) / 32) * nt * 2048 + 8 * Cin + 4096 + 8192 > 150 * 1024) return false;   // all weights must fit in LDS
    *t = ConvTile{1, 1, 0, mt, nt, 4, 1};
    return true;
}

bool conv1x1_launch_info(int Cin, int Cout, int B, int OH, int OW, const ConvTile& t, int persist_wgs, int att_mode, ConvLaunchInfo* o) {
    const Conv1Tile g{t.mt, t.nt, t.pl == 1 ? 1 : 2};
    o->tiles_x = (OH * OW + g.bm - 1) / g.bm; o->tiles_y = 1;
    o->grid_y = Cout / (t.nt * 16);
    o->wgs_per_img = conv16_wgs_per_img(o->tiles_x, B, o->grid_y, persist_wgs);
    o->grid_x = B * o->wgs_per_img;
    o->ring = 0; o->ppw = 0; o->apw = 0;
    o->lds_bytes = g.lds_bytes(Cin, att_mode);
    return true;
}

hipError_t conv1x1_launch(const ConvArgs& a, const ConvTile& t, hipStream_t s) {
    if (a.C0 % 16 || a.C1 % 16) return hipErrorInvalidValue;  // whole 16-channel blocks per source (channel-blocked activations)
    if (a.att_mode != ATT_NONE) {
        // the hand-off's geometry: heads x D channels, D a multiple of 32 (a K step / a 16-channel tile stays inside one head)
        if (a.att_D % 32 || a.att_heads != 2 || a.att_ksplit > C1_MAX_SPLIT) return hipErrorInvalidValue;
        if (a.att_mode == ATT_PART_IN && (a.C1 != 0 || a.C0 != a.att_heads * a.att_D || a.prologue != PRO_RAW || a.gn_tot0 != nullptr)) return hipErrorInvalidValue;
        if (a.att_mode == ATT_QKV_OUT && (a.Cout != 3 * a.att_heads * a.att_D || a.resid != nullptr || a.stat_tot != nullptr)) return hipErrorInvalidValue;
    }
    if (t.pl != 1 && t.pl != 2) return hipErrorInvalidValue;
#define X(mt_, nt_)                                                                                                                   \
    if (t.mt == mt_ && t.nt == nt_) {                                                                                                 \
        if (a.att_mode == ATT_QKV_OUT) return t.pl == 2 ? launch1<mt_, nt_, ATT_QKV_OUT, 2>(a, s) : launch1<mt_, nt_, ATT_QKV_OUT, 1>(a, s); \
        if (a.att_mode == ATT_PART_IN) return t.pl == 2 ? launch1<mt_, nt_, ATT_PART_IN, 2>(a, s) : launch1<mt_, nt_, ATT_PART_IN, 1>(a, s); \
        return t.pl == 2 ? launch1<mt_, nt_, ATT_NONE, 2>(a, s) : launch1<mt_, nt_, ATT_NONE, 1>(a, s);                               \
    }
    X(2, 3) X(1, 3) X(2, 2) X(1, 2) X(2, 1) X(1, 1)
#undef X
    return hipErrorInvalidValue;
}

}  // namespace midd
