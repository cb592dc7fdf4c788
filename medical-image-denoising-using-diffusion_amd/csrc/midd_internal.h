// Internal declarations shared by the HIP kernels and the C-ABI host side of libmidd.so.
// Activations inside the library are fp32, channels innermost; only the boundary tensors ([B,in_channels,H,W],
// in_channels == 1 in every reference call site) are NCHW.  Two layouts:
//   fp32-MFMA plans   NHWC            [B][H][W][C]
//   split-fp16 plans  CHANNEL-BLOCKED [B][C/16][H][W][16]   (round 3)
// The f16x3 kernels stage a K chunk of 16 channels at a time.  In NHWC that is 64 bytes of every pixel's C*4-byte row while L2
// fetches whole 128-byte lines (a chunk pass alone moves twice its bytes: rocprofv3 FETCH_SIZE calibrated on this very
// pattern, tools/mb/fetch_calib.hip), the MFMA tiles of the epilogue leave as 64-byte pieces C*4 bytes apart, and so do the
// residual rows.  Blocked, the chunk of a halo row is one contiguous run, a 16-pixel x 16-cout MFMA tile leaves as ONE contiguous
// KiB, residual rows and the pointwise kernels move whole runs.  Per launch at batch 4, 256x256 (tools/traffic_per_op.sh, L2-side
// bytes): conv2's fetch 128 -> 115 MB (its residual rows), out_conv 100 -> 64 MB for a 50 MB tensor; the 3x3 kernel's own
// chunk reads were already close to halo-only (66.5 -> 64.3 MB: the L2 kept the other half of the lines for the next pass).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "stats_common.h"

namespace midd {

// Launches that ask for more than 64 KB of dynamic LDS must raise the kernel's limit first, once per (kernel instantiation,
// device): `raised` is the instantiation's own static table, zero-initialised, indexed by device (the caches were per
// process).  Returns hipSuccess when `bytes` is already allowed.
constexpr int MIDD_MAX_DEVICES = 64;
inline hipError_t ensure_dynamic_lds(const void* kernel, int bytes, int (&raised)[MIDD_MAX_DEVICES]) {
    if (bytes <= 64 * 1024) return hipSuccess;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= MIDD_MAX_DEVICES) return hipErrorInvalidDevice;
    if (bytes > raised[dev]) {
        e = hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e != hipSuccess) return e;
        raised[dev] = bytes;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------- implicit-GEMM convolution
enum Prologue { PRO_RAW = 0, PRO_GN = 1, PRO_GN_SILU = 2 };

// element index of (sample b, pixel pix, channel ch) in an activation tensor of C channels and HW pixels per sample
__host__ __device__ inline size_t act_index(int blocked, int b, int C, int HW, int pix, int ch) {
    return blocked ? (((size_t)b * (C >> 4) + (ch >> 4)) * HW + pix) * 16 + (ch & 15) : ((size_t)b * HW + pix) * C + ch;
}

struct ConvArgs {          // (activation pointers: NHWC for the fp32-MFMA kernels, channel-blocked for the f16x3 kernels)
    const float* src0;      // C0 channels
    const float* src1;      // C1 channels (virtual torch.cat on dim=1); may be null when C1 == 0
    int C0, C1;
    int B, H, W;            // input spatial size
    int OH, OW;             // output spatial size
    const float* wpack;     // [Cin/16][taps][Cout/16][64 lanes][4]  (MFMA A-fragment order)
    const float* bias;      // [Cout]
    int Cout;
    // GroupNorm of the INPUT (prologue != RAW): per-channel fixed-point (sum, sum of squares) totals of the two
    // concatenated sources, [B][C0/bs0][rep][2][3] / [B][C1/bs1][rep][2][3] limbs, accumulated by the producers (stats_common.h); every
    // workgroup derives scale = rstd*gamma, shift = beta - mean*rstd*gamma of its sample in its prologue
    // prologue == RAW (f16x3 kernels): the same totals, when present, give the operand's power-of-two prescale
    // (raw_prescale_exp, stats_common.h); gn_tot0 == null: the fixed prescale raw_scale_fixed
    const stat_word* gn_tot0; const stat_word* gn_tot1;
    int gn_bs0, gn_bs1;     // channels per totals block of each source (whole blocks per GroupNorm group)
    float raw_scale_fixed;  // f16x3, prologue == RAW without totals: 2^s applied to the operand (out_scale undoes it)
    int* status;            // device word of the workspace: bit MI_STATUS_* set when a kernel meets a non-finite statistic / an operand beyond fp16 (may be null)
    const float* gn_gamma; const float* gn_beta; float gn_eps; double gn_inv_n;      // affine [Cin], eps, 1 / (pixels * channels per group)
    int prologue;
    const float* temb;      // time table [rows][temb_stride], already offset to this block's column
    int temb_stride;
    const int* trow;        // [B] table row per sample
    const float* resid;     // [B][OH][OW][Cout] (layout as above) added in the epilogue, or null
    float* out;             // [B][OH][OW][Cout] (layout as above)
    float out_scale;        // f16x3 only: 2^-(k+s) undoing the operand prescales (1 for fp32)
    // optional fused GroupNorm statistics of the OUTPUT: every workgroup adds the per-channel sum / sum of squares of
    // the pixels it produced to the totals [B][Cout/bs][rep][2][3] (exact integer atomics, stats_common.h); zeroed per forward
    stat_word* stat_tot;
    int stat_rep;           // copies of every totals block of this program (stats_common.h), also for gn_tot0/1
    int stat_bs;            // channels per totals block of the OUTPUT
    // res_conv folded into conv2 (f16x3 3x3 kernel; res_steps == 0 everywhere else): after a tile's 3x3 steps the kernel runs
    // res_steps more K steps of 32 channels each -- the 1x1 res_conv over the BLOCK INPUT (res_src0 [, res_src1]: the virtual
    // torch.cat), operands straight from global memory as in conv1x1_f16x3.hip -- into the same accumulators (rescaled by the
    // power of two between the two products' prescales).  wpack holds the 3x3 steps followed by the res steps; bias is the sum
    // of both biases; res_tot* are the block input's totals (per-sample operand prescale, stats_common.h)
    const float* res_src0; const float* res_src1;
    int res_C0, res_C1, res_steps;
    float res_scale;        // 2^-k of the res_conv weights
    const stat_word* res_tot0; const stat_word* res_tot1;
    int res_bs0, res_bs1;
    // attention hand-off of the f16x3 1x1 kernel (conv1x1_f16x3.hip; att_mode == ATT_NONE everywhere else)
    //   ATT_QKV_OUT  (the qkv projection): q goes to `out` as fp32 [B][N][C]; k and v are written as the split-fp16 images
    //                the attention kernel stages, att_k / att_v [B][heads][hi|lo][Npad][D] (x 2^4), keys >= N zeroed
    //   ATT_PART_IN  (the output projection): the operand is the attention kernel's key-split partials,
    //                src0 = part_o [ksplit][B][N][C] (unnormalised), att_ml [ksplit][B][heads][N][2] = (m, l); the splits
    //                are extra K steps, each element scaled by 2^(m_s - M) / (L 2^14) of its (pixel, head, split) on load
    int att_mode;
    _Float16* att_k; _Float16* att_v;
    const float* att_ml;
    int att_heads, att_D, att_npad, att_ksplit;
    int tiles_x, tiles_y;
    int wgs_per_img;        // f16x3: persistent workgroups per sample (each walks tiles j, j+wgs_per_img, ...)
    int persist_wgs;        // f16x3: persistent-workgroup target of the launch (0 = default)
#ifdef MIDD_CONV_TIMING
    int dbg_slot;           // diagnostic build: row of g_conv_timing
#endif
};

struct ConvTile {           // which template instance to launch
    int ks, stride, tw, mt, nt, wm, wn;
    int cb = 0;             // f16x3 3x3: 16-channel blocks per K chunk (0: conv16_cb(ks)); selects the weight packing too
    int pl = 2;             // fp16-MFMA kernels: planes per operand, 2 = split-fp16 ("f16x3"), 1 = one-product fp16 ("f16"); selects kernel and packing
};

enum AttMode { ATT_NONE = 0, ATT_QKV_OUT = 1, ATT_PART_IN = 2 };
enum StatusBits { STATUS_NONFINITE = 1, STATUS_FP16_RANGE = 2,          // == MI_STATUS_* (include/midd.h)
                  STATUS_DMA_EARLY = 4 };      // diagnostic builds only (-DMIDD_DMA_CHECK, tools/dma_check.sh): data used before its counted wait had covered it

// Picks a tile for (Cout, output pixels, kernel size, stride); returns false if unsupported.
bool conv_pick_tile(int Cout, int B, int OH, int OW, int ks, int stride, ConvTile* t);
hipError_t conv_launch(const ConvArgs& a, const ConvTile& t, hipStream_t s);

// split-fp16 variant (conv_mfma_f16x3.hip): same arguments, weights packed by pack_conv_f16x3
bool conv16_pick_tile(int Cin, int Cout, int B, int OH, int OW, int ks, int stride, ConvTile* t, bool allow_wide = false, int planes = 2);
int conv16_wgs_per_img(int tiles, int B, int ny, int target = 0);   // target 0: 768
bool conv1x1_pick_tile(int Cin, int Cout, int B, int OH, int OW, ConvTile* t);   // ConvTile::tw == 0 marks it
hipError_t conv1x1_launch(const ConvArgs& a, const ConvTile& t, hipStream_t s);      // persistent workgroups per sample (f16x3 kernels)
hipError_t conv16_launch(const ConvArgs& a, const ConvTile& t, hipStream_t s);
// launch geometry of an f16x3 convolution, host only (mi_debug_plan_dump; tests that pin which instantiations a shape reaches)
struct ConvLaunchInfo { int grid_x, grid_y, wgs_per_img, tiles_x, tiles_y, ring, ppw, apw, lds_bytes; };
bool conv16_launch_info(int Cin, int Cout, int B, int OH, int OW, const ConvTile& t, int persist_wgs, ConvLaunchInfo* out);
bool conv1x1_launch_info(int Cin, int Cout, int B, int OH, int OW, const ConvTile& t, int persist_wgs, int att_mode, ConvLaunchInfo* out);
// 16-channel blocks staged per K chunk of the f16x3 kernel (shared with the host packer).
//   3x3: 1 -> 16 channels per chunk, two taps per MFMA step, half the activation LDS of a 32-channel chunk, i.e. three
//             resident workgroups per CU.  Nine taps leave one half step over per block: blocks are walked in PAIRS
//             (c even, c + 1) of 4 + 5 steps, the first step of block c + 1 carrying tap 8 of block c in its lower half
//             (conv16_pair_walk); only an unpaired last block (Cin = 48, 144) keeps a zero-weight half step
//   1x1: 2 -> 32 channels per chunk and step (no halo, so the image is small; halves the number of
//             chunk hand-overs, which dominate a 1x1)
//   3x3, "wide" (cb = 2, picked per launch where the grid leaves at most ~2 workgroups per CU anyway: the 32x32 / 64x64 maps
//             at small batches): 32 channels per chunk, one tap per step -- 9 full steps instead of 2 x 5 (no zero-weight
//             half step) and half the chunk hand-overs; weights packed in that K order as a second copy (pack_conv_f16x3)
__host__ __device__ constexpr int conv16_cb(int ks) { return ks == 1 ? 2 : 1; }
// number of 32-wide K steps the f16x3 kernel walks for (Cin, taps) with cb blocks per chunk (0: the default of the kernel size)
// (the ONE place that says how many steps a K order has: the kernel, the weight packer and the mi_debug_conv16_steps hook
// ask here; the planner and the plan dump do not count K steps.  cb == 1 exists for the 3x3 only.)
__host__ __device__ constexpr bool conv16_pair_walk(int taps, int cb) { return cb == 1 && taps == 9; }
__host__ __device__ inline int conv16_num_steps(int Cin, int taps, int cb = 0) {
    const int nblk = Cin / 16;
    if (cb == 0) cb = conv16_cb(taps == 1 ? 1 : 3);
    // wide chunks: a pair of blocks is `taps` full steps; pair walk: a pair of blocks is 4 + 5 steps.  Either way an
    // unpaired last block takes (taps + 1) / 2 steps, the last one half empty
    const int full = nblk / 2, half = nblk & 1;
    return full * taps + half * ((taps + 1) / 2);
}

// ---------------------------------------------------------------- GroupNorm statistics (stats_common.h)
constexpr int GN_GROUPS_ = 8;                  // nn.GroupNorm(8, C) everywhere in the reference (DDIMModel.py:116,121,139,214)
// per-channel totals of an activation tensor (either layout: `blocked`) no MFMA conv produced (in_conv output, bilinear 2x outputs): `rows` blocks per
// sample each add their partial sums to tot [B][C/bs][rep][2][3]
hipError_t chan_total_launch(const float* src, stat_word* tot, int rep, int bs, int B, int HW, int C, int rows, int blocked, hipStream_t s);
int chan_partial_rows(int HW, int C);
// chan_total_kernel's dynamic LDS: the fp64 partial sums [ppi][C][2] of ppi = 256 / (C / 4) pixel lanes, then the publish accumulators
// (C + 2) x STAT_WORDS.  The kernel does not raise its limit (64 KB); 0: no launch for this width (C % 4, or more than 256 quads).
// The launch allocates by it and the planner refuses a topology whose materialised ConvTranspose would not fit: 1024 channels
// take 65632 bytes.
constexpr size_t CHAN_TOTAL_LDS_LIMIT = 64 * 1024;
inline size_t chan_total_lds_bytes(int C) {
    if (C < 4 || C % 4 || C / 4 > 256) return 0;
    const int ppi = 256 / (C / 4);
    return (size_t)ppi * C * 2 * sizeof(double) + (size_t)(C + 2) * STAT_WORDS * sizeof(stat_word);
}

// ---------------------------------------------------------------- pre/post-processing (prepost.hip)
size_t resize_workspace_bytes(int n, int sw, int sh, int dw, int dh);
hipError_t resize_bicubic_u8_launch(const unsigned char* src, int n, int sw, int sh, unsigned char* dst, int dw, int dh, void* ws, hipStream_t s);
hipError_t u8_to_unit_launch(const unsigned char* src, float* dst, size_t count, hipStream_t s);
hipError_t unit_to_u8_launch(const float* src, unsigned char* dst, size_t count, hipStream_t s);
// float (Pillow 32bpc) resample with a typed load and store (MI_PIX_*), and the 16-bit element conversions
size_t resize_f32_workspace_bytes(int n, int sw, int sh, int dw, int dh);
hipError_t resize_bicubic_f32_launch(const void* src, int src_type, int n, int sw, int sh, void* dst, int dst_type, int dw, int dh,
                                     int clamp, void* ws, hipStream_t s);
hipError_t u16_to_unit_launch(const uint16_t* src, float* dst, size_t count, hipStream_t s);
hipError_t unit_to_u16_launch(const float* src, uint16_t* dst, size_t count, hipStream_t s);
// the window (include/midd.h: THE WINDOW): histogram [n][65536], levels [n][2] from percentiles, the element rules under them
hipError_t histogram_u16_launch(const uint16_t* src, int n, size_t count, uint32_t* hist, hipStream_t s);
hipError_t window_levels_launch(const uint32_t* hist, int n, double p_lo, double p_hi, int32_t* levels, hipStream_t s);
hipError_t window_u16_to_f32_launch(const uint16_t* src, const int32_t* levels, int n, size_t count, float* dst, hipStream_t s);
hipError_t window_f32_to_u16_launch(const float* src, const int32_t* levels, int n, size_t count, uint16_t* dst, hipStream_t s);
hipError_t resize_bicubic_f32_window_launch(const void* src, int src_type, int n, int sw, int sh, void* dst, int dst_type, int dw, int dh,
                                            int clamp, const int32_t* levels, void* ws, hipStream_t s);
size_t metrics_workspace_bytes(int n, int h);
hipError_t metrics_launch(const float* target, const float* pred, int n, int h, int w, double* out, void* ws, hipStream_t s);

// ---------------------------------------------------------------- attention
// qkv: NHWC [B][N][3C], channel = s*C + head*D + d (s in q,k,v);  out: [B][N][C]
hipError_t attention_launch(const float* qkv, float* out, int B, int N, int C, int heads, hipStream_t s);
// split-fp16 variant (attention_f16x3.hip).  Three launches per attention block: the qkv projection's epilogue writes q (fp32
// [B][N][C]) and the split-fp16 images of k and v, the attention kernel leaves key-split partials, the output projection
// combines them while it loads its operand.  Scratch layout (attention16_layout): K image, V image, partial O, partial (m, l).
struct Att16Layout { size_t k_off, v_off, po_off, ml_off, bytes; int npad; };
Att16Layout attention16_layout(int B, int N, int C, int planes = 2);      // planes: fp16 planes of the K / V images (2 = f16x3, 1 = f16)
// split_B: the batch the key split is chosen for (B, or 1 for batch-invariant plans)
hipError_t attention16_launch(const float* q, const _Float16* Kp, const _Float16* Vp, float* part_o, float* part_ml,
                              int B, int ksplit, int tiles_per_split, int N, int C, int heads, hipStream_t s, int planes = 2);
// key split of the f16x3 attention for N keys: splits and 32-key tiles per split (every split owns >= 1 tile)
void attention16_split(int N, int heads, int split_B, int* ksplit, int* tiles_per_split);
bool attention_supported(int head_dim);

// ---------------------------------------------------------------- small direct kernels
// in_conv: Conv3x3 on cat[x, cond] (NCHW [B,ic,H,W] each) -> [B][H][W][Cout] activations (NHWC, or channel-blocked when `blocked`)
// tot != nullptr: also leaves the GroupNorm totals of the output [B][Cout/bs][rep][2][3] (stats_common.h)
hipError_t in_conv_launch(const float* x, const float* cond, const float* w /*[9][2ic][Cout]*/, const float* bias,
                          float* out, stat_word* tot, int rep, int bs, int B, int ic, int H, int W, int Cout, int blocked, hipStream_t s);
// LDS of the two kernels at the ends of the network, in bytes.  Neither raises its kernel's limit, so a workgroup has
// POINTWISE_LDS_LIMIT for its static and dynamic LDS together.  These are the ONE place that says how much a (channels, width)
// pair takes: the launches allocate by them and mi_unet_plan_create refuses a network that would not fit (the sizes depend on
// in_channels and the two widths alone, not on B, H, W), so what plans also launches.
constexpr size_t POINTWISE_LDS_LIMIT = 64 * 1024;
// in_conv1_kernel (one input channel) is instantiated for these widths and sizes its own LDS (it raises its limit where needed)
__host__ __device__ constexpr bool in_conv1_width(int Cout) { return Cout == 32 || Cout == 48 || Cout == 64; }
// in_conv_kernel, all dynamic: weights [9][2ic][Cout] and bias [Cout], the statistics scratch [2][Cout][ppi] of
// ppi = 256 / (Cout / 16) pixel lanes (+ 2 floats of alignment slack), the publish accumulators (Cout + 2) x STAT_WORDS
__host__ __device__ inline size_t in_conv_lds_bytes(int ic, int Cout) {
    const int ppi = 256 / (Cout / 16);
    return (size_t)(9 * 2 * ic * Cout + Cout + 2 * Cout * ppi + 2) * sizeof(float) + (size_t)(Cout + 2) * STAT_WORDS * sizeof(stat_word);
}
// out_conv_*_kernel: a 16 x 16 output tile, its 18 x 18 halo staged 16 channels at a time with a padded pixel stride of 20 floats
// (static), then the weights [ic][9][C] and the GroupNorm scale / shift [2][C] (dynamic)
constexpr int OC_T = 16;
constexpr int OC_I = OC_T + 2;
constexpr int OC_PS = 20;         // padded pixel stride in floats
__host__ __device__ constexpr size_t out_conv_static_lds_bytes() { return (size_t)OC_I * OC_I * OC_PS * sizeof(float); }
__host__ __device__ inline size_t out_conv_dynamic_lds_bytes(int ic, int C) { return ((size_t)ic * 9 * C + 2 * (size_t)C) * sizeof(float); }
__host__ __device__ inline size_t out_conv_lds_bytes(int ic, int C) { return out_conv_static_lds_bytes() + out_conv_dynamic_lds_bytes(ic, C); }

struct OutConvArgs {
    const float* src;       // [B][H][W][C], or channel-blocked [B][C/16][H][W][16] when `blocked`
    int blocked;
    const stat_word* gn_tot; int stat_rep, gn_bs; const float* gn_gamma; const float* gn_beta; float gn_eps;   // GroupNorm of src: totals [B][C/bs][rep][2][3], affine [C]
    const float* w;         // [ic][9][C]
    const float* bias;      // [ic]
    int B, H, W, C, ic;
    float* eps_out;         // NCHW [B,ic,H,W] raw network output, or null
    // fused sampler update (DDIMModel.py:278-284) when x != null:  x <- clamp(c1*(x - c2*clamp(eps)) + c3*noise, 0, 1)
    float* x;               // NCHW [B,ic,H,W], updated in place
    const float* noise;     // NCHW or null
    float c1, c2, c3;
    int clamp_eps;
    // seeded != 0 (needs x): the noise term is drawn in the update instead of read from `noise` (step_noise_common.h):
    // value = f(seed, image, iter, element index inside the sample, member) -- out_conv_seeded_kernel.  Sample b of the launch is
    // VIRTUAL sample v = v0 + b of an image-major (image, member) batch with `members` draws per image:
    // image = sample_offset + v / members, member = member_offset + v % members.  A plain seeded run is members == 1,
    // member_offset == 0: image = sample_offset + v0 + b, member 0.
    int seeded;
    int iter;                       // position in t_list
    unsigned long long seed;
    long long sample_offset;        // global index of the call's image 0
    int v0;                         // virtual index of this launch's sample 0 inside the call
    int members;                    // >= 1
    unsigned member_offset;         // member index of the call's member 0 (member_offset + members <= 2^32)
    // tiles_x != 0 (mi_denoise_tiled): the virtual batch is (image, tile) instead -- `members` = tiles_y * tiles_x tiles per
    // image, tile k = v % members = ky * tiles_x + kx, every draw is member `member_offset` -- and the element index is the
    // pixel's index in the WHOLE image [ic, img_H, img_W] at the tile's origin (tile_geometry.h: tile_origin of ky / kx with
    // this launch's H, W as the tile): the noise field belongs to the image, not to the tiling.  0: pitch W, plane H*W, origin 0
    int tiles_x, tiles_y, img_H, img_W;
};
// mi_denoise_slots: every sample of a launch is a SLOT at its own timestep.  One record per sample and row of the loop, written
// by the host for this row (slot_fill_launch) and read by out_conv_slots_kernel through scalar loads (b is per workgroup).
enum SlotBits { SLOT_ACTIVE = 1, SLOT_NOISE = 2 };      // NOISE: t > 0 and the call has a noise term (seeded or a tensor)
// A slot is a VIRTUAL sample (mi_denoise_slots_virtual): it carries the member word and the frame that out_conv_seeded_kernel
// derives from a.members / a.tiles_x for a uniform launch -- element index = oc * plane + y * pitch + x + origin, all uint32.
// (0, W, H*W, 0) is a whole image, member 0: mi_denoise_slots.  Twelve words, 16-byte aligned: the kernel reads the first quad
// (which decides whether the workgroup leaves) with one s_load_dwordx4 and, past the idle branch, the counter words with an
// s_load_dwordx2 and an s_load_dwordx4 (profiles/slot_tickets_isa.txt).
struct alignas(16) SlotRec {
    float c1, c2, c3;               // x <- clamp(c1 * (x - c2 * eps) + c3 * noise, 0, 1) at the slot's timestep
    int active;                     // SlotBits; 0 = idle: x keeps its bits, nothing is drawn or written
    unsigned iter;                  // noise counter word c2: iter_base + row
    unsigned image;                 // noise counter word c1: low word of the slot's global sample index
    int trow;                       // the slot's time-table row (0 when idle)
    unsigned member;                // noise counter word c3: the slot's ensemble member
    unsigned pitch, plane, origin;  // the element index's frame: row pitch, channel plane and first element of the slot in its image
    int pad;
};
static_assert(sizeof(SlotRec) == 48, "out_conv_slots_kernel reads a record as 12 words");
constexpr int SLOTS_PER_LAUNCH = 32;
struct SlotRecs { SlotRec v[SLOTS_PER_LAUNCH]; };      // 1.5 KiB of kernel arguments (the limit is 4 KiB)
hipError_t slot_fill_launch(int* trow, SlotRec* dst, const SlotRecs& recs, int n, hipStream_t s);
// mi_denoise_slots_rule: the slot's record under THE DDIM UPDATE / THE DPMPP2M UPDATE (include/midd.h), read by out_conv_slots_rule_kernel
// alone; SlotRec and out_conv_slots_kernel are what they were.  `active` takes two more bits: LAST, the slot's list ends with this row
// (the result is clamped to [0, 1]), and HIST, g != 0 (the slot's previous predicted image is read).  Sixteen words, 16-byte aligned,
// the quad that decides whether the workgroup leaves first: one scalar load before the idle branch (hipcc narrows it to `active`
// alone), the coefficients and counter words past it as s_load_dwordx8 + s_load_dwordx4 (profiles/slots_rule_isa.txt).  The coefficients are one row of mi_update_row for the slot's (previous, own, next) timesteps.
enum SlotRuleBits { SLOT_LAST = 4, SLOT_HIST = 8 };
struct alignas(16) SlotRuleRec {
    int active;                     // SlotBits | SlotRuleBits; 0 = idle: x and x0_hist keep their bits, nothing is drawn or written
    int trow;                       // the slot's time-table row (0 when idle)
    unsigned iter;                  // noise counter word c2: iter_base + row
    unsigned image;                 // noise counter word c1: low word of the slot's global sample index
    float k0, k1, r0, r1;           // as DdimCoef
    float a, b, s, g;               // as DdimCoef / DpmCoef; g == 0 under the DDIM rule
    unsigned member;                // noise counter word c3: the slot's ensemble member
    unsigned pitch, plane, origin;  // the element index's frame, as SlotRec's
};
static_assert(sizeof(SlotRuleRec) == 64, "out_conv_slots_rule_kernel reads a record as 16 words");
struct SlotRuleRecs { SlotRuleRec v[SLOTS_PER_LAUNCH]; };      // 2 KiB of kernel arguments (the limit is 4 KiB)
hipError_t slot_rule_fill_launch(int* trow, SlotRuleRec* dst, const SlotRuleRecs& recs, int n, hipStream_t s);
// The DDIM(eta) update (include/midd.h: THE DDIM UPDATE): one row of the host's coefficient table and the launch-uniform switches,
// a kernel argument of out_conv_ddim_kernel / out_conv_ddim_seeded_kernel alone (scalar loads).  OutConvArgs does not grow:
// a.c1 .. a.c3 are not read by these kernels, everything else is.
struct DdimCoef {
    float k0, k1, r0, r1, a, b, s;  // 1/sqrt(A), sqrt(1-A), sqrt(A), 1/sqrt(1-A), sqrt(P), sqrt(max(0, 1-P-sigma^2)), 2 sigma
    int clip_x0;                    // clip the predicted image to [0, 1] and re-derive eps
    int last;                       // last row of the list: the result is clamped to [0, 1]
};
// The second-order multistep update (include/midd.h: THE DPMPP2M UPDATE): the DDIM row at eta = 0 (s == 0 is not carried) and the
// multistep weight g, a kernel argument of out_conv_dpm_kernel alone (scalar loads).  OutConvArgs does not grow here either.
struct DpmCoef {
    float k0, k1, r0, r1, a, b;     // as DdimCoef
    float g;                        // sqrt(P) (1 - e^-h) / (2 max(r, 1)); 0 on the first and the last row: x0_prev is not read
    int clip_x0;
    int last;
};
// The update a step's out_conv launch runs, from the sampler's schedule to the kernel: which rule, and that rule's arguments alone.
//   OUT_FORWARD   : none -- the network output only (mi_unet_forward; a.x is null)
//   OUT_REFERENCE : the reference's, a.c1 .. a.c3 <- ref (the other rules do not read them)
//   OUT_DDIM      : a.seeded != 0 (host: only with k.s > 0): the term s * noise is drawn as out_conv_seeded_kernel draws it; else it
//                   is read from a.noise when that is given and k.s > 0
//   OUT_DPM       : x0_prev (read when k.g != 0) and x0_out (written) are [a.B, ic, H, W] fp32 and may be the same address: each thread
//                   reads its own element before it writes it.  The rule is deterministic: a.seeded or a.noise is refused
//   OUT_SLOTS     : every sample from its record of this row (device, [a.B])
//   OUT_SLOTS_RULE: every sample from its SlotRuleRec of this row (device, [a.B]); clip_x0 is launch-uniform.  x0_hist [a.B, ic, H, W]
//                   is null under the DDIM rule; under the multistep rule it is read where a record has SLOT_HIST, written for every
//                   active slot, in place (each thread reads its own element before it writes it), and a noise source is refused
enum OutUpdateKind { OUT_FORWARD, OUT_REFERENCE, OUT_DDIM, OUT_DPM, OUT_SLOTS, OUT_SLOTS_RULE };
struct RefCoef { float c1, c2, c3; };
struct DpmStep { DpmCoef k; const float* x0_prev; float* x0_out; };
struct SlotRuleStep { const SlotRuleRec* recs; int clip_x0; float* x0_hist; };
struct OutUpdate {
    OutUpdateKind kind;
    union { RefCoef ref; DdimCoef ddim; DpmStep dpm; const SlotRec* slots; SlotRuleStep slots_rule; };
};
hipError_t out_conv_launch(const OutConvArgs& a, const OutUpdate& u, hipStream_t s);
// the kernel symbol that launch runs (without its <1> / <0>): what a profile reports
const char* out_conv_symbol(const OutUpdate& u, int seeded);
// dst [n_iters][B][chw] <- the 0.5-scaled seeded step noise of `member` (step_noise_common.h); chw < 2^32, B and n_iters <= 65535
hipError_t step_noise_fill_launch(float* dst, int n_iters, int B, unsigned long long chw, unsigned long long seed, long long sample_offset,
                                  unsigned member, hipStream_t s);
// The training objective as an evaluation (diffusion_loss.hip; include/midd.h: THE FORWARD NOISE, THE NOISING, THE DENOISING LOSS).
// A sample's record: a = sqrtf(alpha_hat[t]), s = sqrtf(1 - alpha_hat[t]) (host, fp32) and the counter words c1 and c2 (without the top bit) of its forward noise.
// The records of up to LOSS_RECS_PER_LAUNCH consecutive samples travel as kernel arguments: a larger batch takes several launches.
struct alignas(16) LossRec { float a, s; uint32_t sample; uint32_t draw; };
constexpr int LOSS_RECS_PER_LAUNCH = 32;
struct LossRecs { LossRec v[LOSS_RECS_PER_LAUNCH]; };      // 512 bytes of kernel arguments
constexpr int LOSS_PATCH = 32;                             // a workgroup of the loss kernel owns a LOSS_PATCH x LOSS_PATCH patch of one channel
constexpr int LOSS_MAX_SIDE = 1 << 30;                     // H, W of the loss calls: (H + 31) stays inside an int; C*H*W < 2^32 bounds the patch count
inline int loss_tiles(int H, int W) { return ((H + LOSS_PATCH - 1) / LOSS_PATCH) * ((W + LOSS_PATCH - 1) / LOSS_PATCH); }
// x_t [B][chw] <- a * clean + s * eps, eps read (eps != null) or drawn (seeded; then eps_out, if given, receives it); recs [B] HOST
hipError_t noise_images_launch(const float* clean, const float* eps, float* x_t, float* eps_out, const LossRec* recs, int B,
                               unsigned long long chw, int seeded, unsigned long long seed, hipStream_t s);
// bytes of the partial sums of loss_terms_launch: double [B][C][tiles][2]
size_t loss_partials_bytes(int B, int C, int H, int W);
// out double [B][3] <- (mse, edge, mse + edge_weight * edge); maps (or null) float [3][B][C][H][W] <- q, g, p.  Explicit form: x_t and
// eps given; seeded form: both null, z and x_t are formed again from (seed, recs[b].sample, recs[b].draw).  part: loss_partials_bytes
hipError_t loss_terms_launch(const float* clean, const float* x_t, const float* eps, const float* eps_pred, const LossRec* recs,
                             int B, int C, int H, int W, int seeded, unsigned long long seed, int clamp_eps,
                             double edge_weight, double* out, float* maps, double* part, hipStream_t s);

// samples [B][K][chw] -> mean [B][chw] and, when std != null (K >= 2), the unbiased std [B][chw]; fixed double-precision
// arithmetic per pixel (ensemble.hip: ensemble_reduce_kernel).  B <= 65535, K >= 1
hipError_t ensemble_reduce_launch(const float* samples, int B, int K, unsigned long long chw, float* mean, float* std, hipStream_t s);
// dst [n][chw] <- noisy[(v0 + j) / K]: the condition image of the n consecutive virtual samples from v0 (one pass of an ensemble)
hipError_t ensemble_broadcast_launch(const float* noisy, float* dst, int v0, int n, int K, unsigned long long chw, hipStream_t s);

// Tiled denoising (tile_geometry.h).  An image [C,H,W] is cut into ny x nx tiles of th x tw with minimum overlaps oy, ox.
struct TileGeom { int C, H, W, th, tw, oy, ox, ny, nx; };
// dst [n][C][th][tw] <- the tiles of the virtual samples v0 .. v0 + n - 1 (v = image * ny*nx + ky * nx + kx) of noisy [B][C][H][W]; n <= 65535
hipError_t tile_extract_launch(const float* noisy, float* dst, const TileGeom& g, int v0, int n, hipStream_t s);
// out [B][C][H][W] <- the window-weighted mean of the tiles [B][ny*nx][C][th][tw] over every pixel; fixed double arithmetic
hipError_t tile_blend_launch(const float* tiles, float* out, int B, const TileGeom& g, hipStream_t s);
// tiles [M][B][ny*nx][C][th][tw] -> mean, unbiased std [B][C][H][W] over the M blended members and the blended members themselves,
// samples [B][M][C][H][W]; each of the three may be null (not all; std needs M >= 2).  The arithmetic of tile_blend_launch per
// member, then of ensemble_reduce_launch over the members.  B * M * ny*nx <= 2^31 - 1
hipError_t tile_blend_reduce_launch(const float* tiles, int B, int M, const TileGeom& g, float* mean, float* std, float* samples, hipStream_t s);
// tiles [B][ny*nx][C][th][tw], IN PLACE: every element <- tile_blend_launch's value of the pixel it lies over; image [B][C][H][W] or
// null <- those values (tile_consensus.hip; include/midd.h: THE CONSENSUS).  One launch, no temporary
hipError_t tile_consensus_launch(float* tiles, float* image, int B, const TileGeom& g, hipStream_t s);

// Per-pixel quantile maps over the members (quantile_common.h; include/midd.h: mi_ensemble_quantiles).  The levels travel as kernel
// arguments; the members of a pixel are sorted in registers, hence the member limit.
constexpr int QUANTILE_MAX_MEMBERS = 64, QUANTILE_MAX_LEVELS = 8;
struct QuantileLevels { double q[QUANTILE_MAX_LEVELS]; int nq; };
// samples [B][K][chw] -> out [B][nq][chw].  B <= 65535, 1 <= K <= 64, 1 <= nq <= 8, every level in [0, 1]
hipError_t ensemble_quantiles_launch(const float* samples, int B, int K, unsigned long long chw, const QuantileLevels& ql, float* out, hipStream_t s);
// tiles [M][B][ny*nx][C][th][tw] -> out [B][nq][C][H][W]: the quantiles of the M blended members (the arithmetic of tile_blend_launch
// per member, then of ensemble_quantiles_launch).  The limits of tile_blend_reduce_launch and of the call above
hipError_t tile_blend_quantiles_launch(const float* tiles, int B, int M, const TileGeom& g, const QuantileLevels& ql, float* out, hipStream_t s);

// Scores of an ensemble against a truth image (ensemble_scores.hip; include/midd.h: THE ENSEMBLE SCORES).  samples [B][K][chw], truth
// [B][chw] -> sums double [B][4] = (A, G, E, V), invalid [B], rank_hist [B][2K+1], counts [B][nq][2] (null iff nq == 0), crps_map
// [B][chw] or null; part: ensemble_scores_partials_bytes, the chunk sums.  Zeroes the integer outputs on the stream.  B <= 65535,
// 1 <= K <= 64, 0 <= nq <= 8, every level in [0, 1]
size_t ensemble_scores_partials_bytes(int B, unsigned long long chw);
hipError_t ensemble_scores_launch(const float* samples, const float* truth, int B, int K, unsigned long long chw, const QuantileLevels& ql,
                                  double* sums, unsigned long long* invalid, unsigned long long* rank_hist, unsigned long long* counts,
                                  float* crps_map, double* part, hipStream_t s);

// Principal modes of an ensemble's spread (ensemble_modes.hip; include/midd.h: THE ENSEMBLE MODES).  samples [B][K][chw] -> gram
// double [B][K][K], symmetric, and invalid [B] (zeroed on the stream); ws: ensemble_gram_workspace_bytes (the chunk sums of the
// packed upper triangle and, for K > 8, the double means).  weights double [B][M][K] on the device -> out [B][M][chw].  B <= 65535,
// 2 <= K <= 64, 1 <= M <= 8
constexpr int MODES_MAX_MEMBERS = 64, MODES_MAX_MODES = 8;
unsigned long long ensemble_gram_chunks(unsigned long long chw);
size_t ensemble_gram_workspace_bytes(int B, int K, unsigned long long chw);
hipError_t ensemble_gram_launch(const float* samples, int B, int K, unsigned long long chw, double* gram, unsigned long long* invalid,
                                double* ws, hipStream_t s);
hipError_t ensemble_project_launch(const float* samples, int B, int K, unsigned long long chw, const double* weights, int M, float* out, hipStream_t s);

// The responses of planes to channel templates (channel_responses.hip; include/midd.h: THE CHANNEL RESPONSES).  x [N][H][W], centres a
// HOST table [L][2] of (cy, cx) whose ROIs of side R all lie inside the image, channels double [C][R][R] on the device -> out double
// [N][L][C], invalid uint32 [N][L].  The origins travel as kernel arguments, 512 locations a launch
constexpr int CR_MAX_PLANES = 65535, CR_MAX_SIDE = 32768, CR_MIN_ROI = 4, CR_MAX_ROI = 128, CR_MAX_LOCATIONS = 4096, CR_MAX_CHANNELS = 32;
hipError_t channel_responses_launch(const float* x, int N, int H, int W, const int32_t* centres, int L, int R, const double* channels, int C,
                                    double* out, uint32_t* invalid, hipStream_t s);

// The noise power spectrum of f = a - b (nps.hip; include/midd.h: THE NOISE POWER SPECTRUM).  a [B][K][C][H][W], b [B][C][H][W] or
// null; R in {32, 64, 128}, S >= 1, detrend 0 none / 1 mean / 2 plane, window a HOST table of R floats or null -> nps double
// [B*C][R][R], radial double [B*C][R/2+1], radial_count [R/2+1], rois_used and rois_skipped [B*C]; ws: nps_workspace_bytes (the chunk
// sums of the half plane, double [B*C][chunks][R*(R/2+1)], then the chunks' used counts).  B*C <= 65535, chunks < 2^31.  The twiddle and
// window tables travel as a kernel argument
constexpr int NPS_CHUNK = 16;
struct NpsTables { float tc[64]; float ts[64]; float w[128]; };
unsigned long long nps_chunks(int K, int H, int W, int R, int S);
size_t nps_workspace_bytes(int groups, int K, int H, int W, int R, int S);
hipError_t nps_launch(const float* a, const float* b, int B, int K, int C, int H, int W, int R, int S, int detrend, const float* window,
                      double scale, int exclude_axes, double* nps, double* radial, long long* radial_count, long long* rois_used,
                      long long* rois_skipped, void* ws, hipStream_t s);
void nps_tables(int R, const float* window, NpsTables* tab, double* sw);

// The Welch cross-spectrum of x [B][Kx][C][H][W] and y [B][Ky][C][H][W], Kx, Ky in {K, 1} (cross_spectrum.hip; include/midd.h: THE
// CROSS SPECTRUM): ROIs, detrend, window and bins as above -> planes double [4][B*C][R][R] (Sxx, Syy, Re Sxy, Im Sxy), radial double
// [4][B*C][R/2+1], radial_count, rois_used, rois_skipped as above; ws: xs_workspace_bytes (four chunk sums per half-plane entry)
size_t xs_workspace_bytes(int groups, int K, int H, int W, int R, int S);
hipError_t xs_launch(const float* x, const float* y, int B, int Kx, int Ky, int C, int H, int W, int R, int S, int detrend, const float* window,
                     int exclude_axes, double* planes, double* radial, long long* radial_count, long long* rois_used, long long* rois_skipped,
                     void* ws, hipStream_t s);

// Geometric self-ensemble (include/midd.h: THE GEOMETRY).  A view list is 1 .. 8 distinct codes g = 4 t + 2 fy + fx in the caller's
// order; it travels as kernel arguments.  Transposing codes (g >= 4) need H == W.
constexpr int DIHEDRAL_MAX_VIEWS = 8;
struct DihedralViews { int n; uint8_t code[DIHEDRAL_MAX_VIEWS]; };
// dst [n][C][Hv][Wv] <- view(images[v / G], code[v % G]) for the virtual samples v = v0 .. v0 + n - 1 (image-major); n <= 65535
hipError_t dihedral_views_launch(const float* images, float* dst, const DihedralViews& dv, int C, int H, int W, int v0, int n, hipStream_t s);
// views_out [B][G][C][Hv][Wv] (every view in its own frame) -> mean, unbiased std [B][C][H][W] over the views turned back and those
// aligned members, samples [B][G][C][H][W]; each of the three may be null (not all; std needs G >= 2).  The arithmetic of
// ensemble_reduce_launch over unview of every view, in list order.  B <= 65535
hipError_t dihedral_reduce_launch(const float* views_out, int B, const DihedralViews& dv, int C, int H, int W,
                                  float* mean, float* std, float* samples, hipStream_t s);
// views_out as above -> out [B][nq][C][H][W]: the arithmetic of ensemble_quantiles_launch over the aligned members
hipError_t dihedral_quantiles_launch(const float* views_out, int B, const DihedralViews& dv, int C, int H, int W,
                                     const QuantileLevels& ql, float* out, hipStream_t s);

// Tiled self-ensemble (tiled_views.hip; include/midd.h: mi_denoise_tiled_self_ensemble).  A transposing view turns H x W into
// W x H here -- H == W is not needed -- and its tiles are those of the viewed image: with a transposing code th == tw, oy == ox.
// dst [B][C][Hv][Wv] <- view(images [B][C][H][W], code), one code per launch: the viewed batch of one round.  B <= 65535
hipError_t plane_view_launch(const float* images, float* dst, int code, int B, int C, int H, int W, hipStream_t s);
// tiles [G][B][ny*nx][C][th][tw] (view k's tiles in ITS frame; g: the geometry of the un-viewed H x W image) -> mean, unbiased std
// [B][C][H][W] over the views blended and turned back and those aligned members, samples [B][G][C][H][W]; each of the three may be
// null (not all; std needs G >= 2).  The arithmetic of tile_blend_launch per view, then of ensemble_reduce_launch.  B <= 65535
hipError_t tile_blend_unview_reduce_launch(const float* tiles, int B, const DihedralViews& dv, const TileGeom& g,
                                           float* mean, float* std, float* samples, hipStream_t s);
// tiles as above -> out [B][nq][C][H][W]: the arithmetic of ensemble_quantiles_launch over the aligned blended members
hipError_t tile_blend_unview_quantiles_launch(const float* tiles, int B, const DihedralViews& dv, const TileGeom& g,
                                              const QuantileLevels& ql, float* out, hipStream_t s);

// bilinear resize of an activation tensor, either layout (align_corners=False), any size ratio
hipError_t resize_bilinear_launch(const float* src, float* dst, stat_word* tot, int rep, int bs, int B, int H, int W, int C, int OH, int OW, int blocked, hipStream_t s);
// ConvTranspose2d(C,C,4,stride=2,padding=1) direct (only used by topologies where it cannot be folded)
hipError_t conv_transpose_launch(const float* src, const float* w /*[4][4][Cin][Cout]*/, const float* bias, float* dst,
                                 int B, int H, int W, int Cin, int Cout, int blocked, hipStream_t s);
// activation tensor (either layout) -> NCHW copy (debug fetch)
hipError_t nhwc_to_nchw_launch(const float* src, float* dst, int B, int H, int W, int C, int blocked, hipStream_t s);
hipError_t fill_i32_launch(int* dst, const int* host_vals, int n, hipStream_t s);

}  // namespace midd
