// What the executor (midd_exec.hip), the sampler calls (midd_sampler.hip), the batched calls (midd_batched.hip) and the stand-alone
// analysis calls (midd_analysis.hip) share.
#pragma once
#include "midd_host.h"

namespace midd {

// The noise term of the cddpm update: none, a caller's tensor (mi_denoise), or drawn in the update (mi_denoise_seeded,
// mi_denoise_ensemble).  Seeded: the B samples of the run are the virtual samples v0 .. v0 + B - 1 of an image-major
// (image, member) batch with `members` draws per image numbered from `member_offset`, image 0 being global image
// `sample_offset`; a plain seeded run is members = 1, v0 = 0 (OutConvArgs, midd_internal.h).
struct StepNoise {
    const float* tensor = nullptr; bool seeded = false; uint64_t seed = 0; int64_t sample_offset = 0;
    int v0 = 0; int members = 1; uint32_t member_offset = 0;
    // mi_denoise_tiled: the virtual samples are (image, tile) pairs, members = tiles_y * tiles_x, and the noise is indexed by the
    // pixel's place in the whole img_H x img_W image (OutConvArgs)
    int tiles_x = 0, tiles_y = 0, img_H = 0, img_W = 0;
};

// the sampler's schedule as a caller gives it: the timestep rows (uniform: t[n]; mi_denoise_slots: a table t[n][B]) and the tables
// and the update rule of the uniform calls (include/midd.h: mi_update_rule, its MI_UPDATE_* kind)
struct Schedule {
    const int32_t* t; int n; const float *beta, *alpha, *alpha_hat; int noise_steps;
    int rule = MI_UPDATE_REFERENCE; double eta = 0.0; int clip_x0 = 1;      // (eta: MI_UPDATE_DDIM's; 0 under every other rule)
    // MI_UPDATE_DPMPP2M (include/midd.h: THE DPMPP2M UPDATE): the caller's history of predicted images, one run's worth
    // [slots][B, C, H, W] -- x0_stride 0: one slot, read and written in place; else the elements between two slots of the trajectory
    float* x0 = nullptr; size_t x0_stride = 0;
};

struct StepIO {
    const float* x; const float* cond; float* eps_out;
    float* x_update; const float* noise; int clamp_eps;
    // the step's update and that rule's own arguments (midd_internal.h: OutUpdate); of the fields above OUT_DPM reads x_update and
    // clamp_eps only, OUT_SLOTS x_update, noise, clamp_eps, sn.seeded and sn.seed only
    OutUpdate update;
    // sn.seeded: the update draws its noise term (step_noise_common.h) for iteration `iter`, sample 0 of THIS program being virtual
    // sample sn.v0; a step that draws nothing keeps the defaults (sn.tensor is not read: `noise` is this step's slice of it)
    int iter; StepNoise sn;
};

// The rows of a sampler call.  Uniform (mi_denoise and its siblings, slots == null): row i puts every sample at sc.t[i], x starts
// as a copy of the condition images.  Slots (mi_denoise_slots): sc.t is a table [n][B], sample b is at t[i * B + b] in row i or
// idle (-1), its noise counter words are (sample_index[b], iter_base[b] + i), and x is the caller's: it is not initialised.
struct SlotRows {
    const int32_t* iter_base;         // [B] or null (all 0)
    const int64_t* sample_index;      // [B] or null (0 .. B-1)
    // mi_denoise_slots_virtual: the slot's member word and the frame of its element index (SlotRec, midd_internal.h)
    const int64_t* member = nullptr;  // [B] or null (all 0)
    const uint32_t* frame = nullptr;  // [B][3] (pitch, plane, origin) or null: (W, H*W, 0)
    // mi_denoise_slots_rule (sc.rule != MI_UPDATE_REFERENCE; sc.x0 is the call's x0_hist [B, C, H, W] under the multistep rule): the
    // slot's timestep before the call's first row and after its last one, -1 = none (SlotRuleRec, midd_internal.h)
    const int32_t* t_before = nullptr;    // [B] or null (all -1)
    const int32_t* t_after = nullptr;     // [B] or null (all -1)
};

// the rc of a launch wrapper's hipError_t
inline int launched(hipError_t e, const char* what) {
    return e == hipSuccess ? MI_OK : fail(MI_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// no two of the n buffers may overlap (a null one is absent); `why` is the call's sentence on who reads and who writes
struct Buf { const void* p; size_t bytes; const char* name; };
int check_no_overlap(const Buf* b, int n, const char* why);                                             // midd_sampler.hip

// midd_analysis.hip: the member, batch and level rules of the reduce and quantile calls, which the batched calls compose
constexpr int64_t MEMBER_WORDS = (int64_t)1 << 32;      // the member index is one 32-bit counter word
int check_members_min(int members);
int check_std_members(const float* std_out, int members);
int check_reduce_batch(int B, const char* why = "limit of the reduce kernel's grid");
int check_quantile_members(int members);
int check_quantile_levels(const double* q, int nq, QuantileLevels* ql, int nq_min = 1);

// midd_exec.hip.  status: the call's status word (first word of the CALLER's workspace, whichever sub-batch program runs)
int run_program(mi_plan* p, Program* g, const StepIO& io, char* ws, int* status, hipStream_t s, hipEvent_t mid_event = nullptr, int mid_div = 2);
int check_device(mi_plan* plan);
int check_finalized(mi_plan* plan);
int check_workspace(const void* ws, size_t got, size_t need);
int check_call(mi_plan* plan, int B, int H, int W, void* ws, size_t ws_bytes, Program** g);

// midd_sampler.hip
int check_schedule(mi_plan* plan, const Schedule& sc);
int apply_rule(const mi_update_rule* rule, Schedule* sc);
int apply_dpm(int clip_x0, float* x0, Schedule* sc);
int check_step_noise_range(int64_t C, int64_t H, int64_t W, int64_t sample_offset);
int check_run(mi_plan* plan, const float* noisy, const float* x_out, int B, int H, int W, const Schedule& sc,
              void* workspace, size_t workspace_bytes, Program** g);
int enqueue_run(mi_plan* plan, Program* g, const float* noisy, float* x_out, int B, int H, int W,
                const Schedule& sc, const SlotRows* slots, const StepNoise& sn, int flags,
                void* workspace, size_t workspace_bytes, void* stream);

}  // namespace midd
