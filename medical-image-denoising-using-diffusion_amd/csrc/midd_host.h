// Types and functions shared by the host side of libmidd.so: midd_abi.hip (C ABI surface), midd_weights.hip (topology, weight
// repacking, time table), midd_planner.hip (execution planner), midd_exec.hip (executor), midd_sampler.hip (sampler calls),
// midd_batched.hip (batched calls), midd_analysis.hip (stand-alone analysis calls) and midd_loss.hip (the denoising-loss calls; the
// last five share midd_sampler.h).  No torch, no allocation on the hot path.
#pragma once
#include "../../include/midd.h"
#include "midd_internal.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

namespace midd {

constexpr int ATTN_HEADS_ABI = 2;       // AttentionBlock(num_heads=2), DDIMModel.py:136
constexpr float ACT_PRESCALE_H = 16.0f; // 2^s: must match ACT_PRESCALE in conv_mfma_f16x3.hip

// sets the thread's mi_last_error text and returns `code` (midd_abi.hip)
int fail(int code, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
#define HIPCHK(expr)                                                                           \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) return fail(MI_EHIP, "%s failed: %s", #expr, hipGetErrorString(e_)); \
    } while (0)

enum ModKind { MOD_RB, MOD_ATTN, MOD_DOWN, MOD_UP };
struct Mod {
    ModKind kind;
    std::string name;
    int in_c, out_c;
    int temb_col = -1;       // column offset into the time table (residual blocks)
    // device offsets (floats) into the packed weight buffer, filled by finalize
    size_t w1 = 0, b1 = 0, w2 = 0, b2 = 0, wr = 0, br = 0;       // rb: conv1, conv2, res_conv
    size_t w1x = (size_t)-1, w2x = (size_t)-1, wcx = (size_t)-1;  // f16x3: the same 3x3 weights in the wide-chunk K order (conv16_pick_tile: cb = 2); -1: none
    size_t b2r = 0;                                               // rb, f16x3, in_c != out_c: conv2's weights carry the res_conv steps (folded); bias sum
    size_t g1 = 0, be1 = 0, g2 = 0, be2 = 0;                      // rb / attn GroupNorm affine
    size_t wq = 0, bq = 0, wp = 0, bp = 0;                        // attn: qkv, proj
    size_t wc = 0, bc = 0, wt = 0;                                // down / up(folded 3x3) conv, raw ConvT
    float s1 = 1.f, s2 = 1.f, sr = 1.f, sq = 1.f, sp = 1.f, sc = 1.f;   // f16x3 output scales of the convs above
};

struct HostWeight { std::vector<int64_t> shape; std::vector<float> data; bool loaded = false; };

struct TensorRef {
    size_t off = 0; int C = 0, H = 0, W = 0;
    // GroupNorm statistics, if produced: per-channel fixed-point totals [B][C][replica][2][3] (stats_common.h), inside the statistics arena
    size_t tot_off = (size_t)-1; int stat_id = -1, stat_bs = 0;      // stat_id: index into the builder's table until the arena is placed
};

struct GnRef { size_t gamma = 0, beta = 0; bool on = false; };        // affine of the GroupNorm in front of a consumer

enum OpKind { OP_IN_CONV, OP_CONV, OP_ATTN, OP_RESIZE, OP_CONVT, OP_OUT, OP_CHAN_TOT };
struct Op {
    OpKind kind;
    // sources / destination (workspace offsets in bytes)
    TensorRef s0, s1, dst, resid;
    bool has_s1 = false, has_resid = false;
    GnRef gn;                   // OP_CONV / OP_OUT: GroupNorm of (s0, s1) applied while staging
    size_t partial_off = 0;     // OP_ATTN and its two projections (f16x3): the attention scratch (attention16_layout)
    int att_mode = ATT_NONE, att_ksplit = 1, att_tps = 1;      // f16x3 attention hand-off (conv1x1_f16x3.hip); key split of the block
    int stat_rows = 0;          // OP_CHAN_TOT: blocks per sample
    // OP_CONV
    size_t w = 0, b = 0;
    int prologue = PRO_RAW, temb_col = -1;
    ConvTile tile{};
    int stride = 1, ks = 3;
    bool want_stats = false;
    TensorRef res0, res1;       // f16x3 conv2 with the res_conv folded in: the block input (virtual cat)
    bool has_res1 = false; int res_steps = 0; float res_scale = 1.f;
    bool raw_stats = false;     // prologue RAW: the sources' totals exist -> per-sample power-of-two prescale (stats_common.h)
    float raw_scale_fixed = 1.f; // prologue RAW without totals: fixed prescale of the operand
    float out_scale = 1.f;
};

// Batch-invariant plans (MI_COMPUTE_BATCH_INVARIANT) make every per-sample decision -- tile, persistent workgroups per
// sample, attention key split, chunk width -- as the DEFAULT plan of a side-by-side sub-batch of this many samples does:
// 4 = one half of BASELINE configs[1]'s batch of 8, so at that batch the invariant plan IS the default plan (no cost), larger
// batches keep the per-image cost of batch 8 (they give up the few per cent a larger batch gains) and a single image runs
// on the 160-workgroup grids of one quarter of a sub-batch.  (Round 2 planned as for a batch of one: -19 % at batch 8.)
constexpr int INVARIANT_B = 4;

struct Program {
    int B, H, W;
    int persist_wgs = 0;       // f16x3 convs: persistent-workgroup target of this program (0 = default)
    bool wide_chunks = false;  // f16x3 3x3 convs may take the wide-chunk variant (conv16_pick_tile): programs that run alone
    std::vector<Op> ops;
    size_t bytes = 0, trow_off = 0;
    size_t slot_off = 0;                        // SlotRec [B] or SlotRuleRec [B] (midd_internal.h; sized for the larger): rewritten before every row of mi_denoise_slots / mi_denoise_slots_rule
    size_t stats_off = 0, stats_bytes = 0;      // statistics arena: every tensor's totals, zeroed by one memset per forward
    int stat_rep = 1;                           // copies per channel (against same-address atomic serialisation)
    std::map<std::string, TensorRef> outputs;
};

// f16x3 plans keep a second, wide-chunk copy (conv16_pick_tile: cb = 2) of a residual block's two 3x3 weights and of a folded
// up-conv's, when the conv has at least one 32-channel chunk: what mi_unet_finalize packs and what the planner may pick
inline bool packs_wide_copy(const mi_unet_cfg& cfg, int Cin) { return cfg.compute_mode != MI_COMPUTE_F32 && Cin >= 32; }
// The two fp16-MFMA modes share planner, layouts (channel-blocked activations) and kernels' structure; they differ in the fp16
// planes every MFMA operand has: 2 = hi | lo, three products (MI_COMPUTE_F16X3); 1 = the rounded value, one product (MI_COMPUTE_F16)
inline bool fp16_mfma(const mi_unet_cfg& cfg) { return cfg.compute_mode == MI_COMPUTE_F16X3 || cfg.compute_mode == MI_COMPUTE_F16; }
inline int operand_planes(const mi_unet_cfg& cfg) { return cfg.compute_mode == MI_COMPUTE_F16 ? 1 : 2; }

int build_topology(mi_plan* p);                                                                   // midd_weights.hip
int get_program(mi_plan* p, int B, int H, int W, Program** out, bool side_by_side = false);       // midd_planner.hip
int split_parts(int B);
void op_work(mi_plan* p, Program* g, const Op& o, std::string* name, double* flops, double* bytes);
int dump_program(mi_plan* p, int B, int H, int W, bool side_by_side, std::string* out);
// mi_denoise_ensemble.  Layout of its workspace: [sampler workspace of a pass | condition images of a pass | member outputs
// (unless the caller gives samples_out)]; pass = virtual samples per pass, tail = those of the last pass when it is shorter (else 0)
struct EnsembleLayout { int pass, tail; size_t run_bytes, cond_off, samples_off, bytes; };
int ensemble_layout(mi_plan* p, int B, int members, int H, int W, int pass_samples, bool samples_external, EnsembleLayout* L);   // midd_planner.hip
int check_ensemble_args(mi_plan* p, int B, int members, int H, int W, int64_t sample_offset, int64_t member_offset, int pass_samples);   // midd_batched.hip
// mi_denoise_tiled: its argument rules (no GPU work) -> the geometry; its workspace is an EnsembleLayout with members = tiles per
// image at the tile's shape: [sampler workspace of a pass | condition tiles of a pass | tile outputs (unless tiles_out is given)]
int check_tiled_args(mi_plan* p, int B, int H, int W, int th, int tw, int oy, int ox, int64_t sample_offset, int pass_samples, TileGeom* g);   // midd_batched.hip
// mi_denoise_tiled_ensemble: the rules of mi_denoise_tiled and of an ensemble's members (no GPU work) -> the geometry; its workspace
// is mi_denoise_tiled's -- a pass never spans two members -- with the tile outputs of every member: [sampler workspace of a pass |
// condition tiles of a pass | tile outputs [members][B][tiles] (unless tiles_out is given)]
int check_tiled_ensemble_args(mi_plan* p, int B, int members, int H, int W, int th, int tw, int oy, int ox, int64_t sample_offset,
                              int64_t member_offset, int pass_samples, TileGeom* g);   // midd_batched.hip
int tiled_ensemble_layout(mi_plan* p, int B, int members, int tiles, int th, int tw, int pass_samples, bool tiles_external, EnsembleLayout* L);   // midd_planner.hip
// mi_denoise_self_ensemble: its workspace is mi_denoise_ensemble's with members = views and the member outputs ALWAYS inside:
// [sampler workspace of a pass | condition views of a pass | view outputs [B][views], each in its view's frame]
// mi_denoise_tiled_self_ensemble: its workspace is mi_denoise_tiled's -- a pass never spans two views -- with the viewed copy of the
// batch of the round that runs and the tile outputs of every view: [sampler workspace of a pass | condition tiles of a pass |
// view(noisy) of one round, B * C*H*W floats rounded up to 256 bytes, at *view_off | tile outputs [views][B][tiles] (unless
// tiles_out is given), at L->samples_off]
int tiled_self_ensemble_layout(mi_plan* p, int B, int n_views, int tiles, int H, int W, int th, int tw, int pass_samples, bool tiles_external,
                               EnsembleLayout* L, size_t* view_off);   // midd_planner.hip
// mi_denoise_tiled_fused: the steps are the outer loop, so the condition tiles of EVERY pass are kept for the whole call:
// [sampler workspace of a pass | condition tiles of all B * tiles virtual samples, at L->cond_off | the tile states (unless tiles_out
// is given), at L->samples_off]
int tiled_fused_layout(mi_plan* p, int B, int tiles, int th, int tw, int pass_samples, bool tiles_external, EnsembleLayout* L);   // midd_planner.hip
}  // namespace midd

struct mi_plan {
    mi_unet_cfg cfg{};                                       // compute_mode holds the arithmetic only (flag bits stripped)
    bool batch_invariant = false;                            // MI_COMPUTE_BATCH_INVARIANT: plan every launch as for a batch of INVARIANT_B
    std::vector<midd::Mod> downs, mid, ups;
    int final_c = 0, temb_cols = 0, levels = 0;
    std::vector<std::string> expected;                       // state-dict key order
    std::map<std::string, std::vector<int64_t>> expected_shape;
    std::map<std::string, midd::HostWeight> host;
    // device side
    float* wdev = nullptr;
    float* ttab = nullptr; int time_rows = 0;
    size_t w_in = 0, b_in = 0, g_out = 0, be_out = 0, w_out = 0, b_out = 0;
    bool finalized = false;
    int device = -1;
    std::mutex mu;
    std::map<uint64_t, std::unique_ptr<midd::Program>> programs;
    // two half-batches on two streams (mi_denoise): side stream + fork / phase / join events
    static const int MAX_PARTS = 4;
    hipStream_t sstream[MAX_PARTS] = {nullptr, nullptr, nullptr, nullptr};        // [0] unused (caller's stream)
    hipEvent_t sev_fork = nullptr, sev_phase[MAX_PARTS] = {nullptr, nullptr, nullptr, nullptr},
               sev_join[MAX_PARTS] = {nullptr, nullptr, nullptr, nullptr};
    std::mutex side_mu;
    // profiling (mi_profile_begin/end)
    bool profiling = false;
    struct Span { hipEvent_t a, b; std::string name; double flops, bytes; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> event_pool;
};
