// The HBM-bound direct kernel at the tail of the UNet, fused with the sampler update, and the fills that feed it.
//
//   out_conv_kernel  : GroupNorm-apply + SiLU + Conv3x3 C -> ic       (DDIMModel.py:213-217,248)
//                      fused with the sampler update of DiffusionDenoiser.denoise
//                      (DDIMModel.py:278-284; cddpm noise term cddpmModels.py:297-303)
//   out_conv_seeded_kernel : the same with the noise term drawn in the update (step_noise_common.h)
//   out_conv_ddim_kernel, out_conv_ddim_seeded_kernel : the same two with the DDIM(eta) update in the place of the reference's
//   out_conv_dpm_kernel    : the same with the second-order multistep update (DPM-Solver++(2M), bounded weight); writes x0
//   out_conv_slots_kernel  : the same with every sample at its own timestep: coefficients, counter words and the active
//                      flag from the sample's SlotRec (mi_denoise_slots); slot_fill_kernel writes a row's records
//   out_conv_slots_rule_kernel : the per-slot form of the DDIM(eta) and multistep updates: the coefficient row, the counter words
//                      and the flags from the sample's SlotRuleRec (mi_denoise_slots_rule)
//   step_noise_fill_kernel : the same noise values as a [n_iters,B,C,H,W] tensor (replay / export)
// N = 1 is a degenerate GEMM shape: it stays on the vector ALU and is judged against the HBM roofline.
#include "midd_internal.h"
#include "pointwise_common.h"
#include "step_noise_common.h"
#include "tile_geometry.h"

namespace midd {

// x * sigmoid(x) on v_exp_f32 / v_rcp_f32 (~1 ulp each)
__device__ __forceinline__ float silu_pw(float v) {
    return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f));
}

// ------------------------------------------------------------------------------ out_conv (+ sampler update)
// Workgroup = 16x16 output pixels.  The 18x18 halo is staged through LDS in 16-channel chunks
// with GroupNorm-apply + SiLU on the way in; pixel stride 20 floats keeps the float4 reads of
// 16 neighbouring lanes on distinct banks.
// (OC_T = 16, OC_I = 18, OC_PS = 20 and the LDS the kernels take: midd_internal.h)

// IC: output channels at compile time (1: the reference's grayscale case; 0: a.ic at run time, <= 4).  With the count
// only known at run time hipcc indexes the accumulators through select chains and splits the 16-byte LDS reads:
// 7 340 instructions, 989 v_cndmask among them, for a loop of 432 multiply-adds (round 3; tools/isa_count.py).
#define MIDD_OUT_SLOTS 0
#define MIDD_OUT_DDIM 0
#define MIDD_OUT_DPM 0
#define MIDD_OUT_SLOTS_RULE 0
#define MIDD_OUT_KERNEL out_conv_kernel
#define MIDD_OUT_SEEDED 0
#include "out_conv_body.h"
#undef MIDD_OUT_KERNEL
#undef MIDD_OUT_SEEDED
#define MIDD_OUT_KERNEL out_conv_seeded_kernel
#define MIDD_OUT_SEEDED 1
#include "out_conv_body.h"
#undef MIDD_OUT_KERNEL
#undef MIDD_OUT_SEEDED
#undef MIDD_OUT_SLOTS
// per-slot update (mi_denoise_slots): coefficients, counter words and the active flag from the sample's SlotRec
#define MIDD_OUT_SLOTS 1
#define MIDD_OUT_KERNEL out_conv_slots_kernel
#define MIDD_OUT_SEEDED 0
#include "out_conv_body.h"
#undef MIDD_OUT_KERNEL
#undef MIDD_OUT_SEEDED
#undef MIDD_OUT_SLOTS
#undef MIDD_OUT_DDIM
// the DDIM(eta) update (include/midd.h: THE DDIM UPDATE): its tensor-noise and its seeded form, coefficients in a DdimCoef argument
#define MIDD_OUT_SLOTS 0
#define MIDD_OUT_DDIM 1
#define MIDD_OUT_KERNEL out_conv_ddim_kernel
#define MIDD_OUT_SEEDED 0
#include "out_conv_body.h"
#undef MIDD_OUT_KERNEL
#undef MIDD_OUT_SEEDED
#define MIDD_OUT_KERNEL out_conv_ddim_seeded_kernel
#define MIDD_OUT_SEEDED 1
#include "out_conv_body.h"
#undef MIDD_OUT_KERNEL
#undef MIDD_OUT_SEEDED
#undef MIDD_OUT_SLOTS
#undef MIDD_OUT_DDIM
#undef MIDD_OUT_DPM
// the second-order multistep update (include/midd.h: THE DPMPP2M UPDATE): deterministic, so one form; coefficients in a DpmCoef argument
#define MIDD_OUT_SLOTS 0
#define MIDD_OUT_DDIM 0
#define MIDD_OUT_DPM 1
#define MIDD_OUT_KERNEL out_conv_dpm_kernel
#define MIDD_OUT_SEEDED 0
#include "out_conv_body.h"
#undef MIDD_OUT_KERNEL
#undef MIDD_OUT_SEEDED
#undef MIDD_OUT_SLOTS
#undef MIDD_OUT_DDIM
#undef MIDD_OUT_DPM
#undef MIDD_OUT_SLOTS_RULE
// the per-slot DDIM(eta) / multistep update (mi_denoise_slots_rule): every per-sample scalar from the sample's SlotRuleRec
#define MIDD_OUT_SLOTS 0
#define MIDD_OUT_DDIM 0
#define MIDD_OUT_DPM 0
#define MIDD_OUT_SLOTS_RULE 1
#define MIDD_OUT_KERNEL out_conv_slots_rule_kernel
#define MIDD_OUT_SEEDED 0
#include "out_conv_body.h"
#undef MIDD_OUT_KERNEL
#undef MIDD_OUT_SEEDED
#undef MIDD_OUT_SLOTS
#undef MIDD_OUT_DDIM
#undef MIDD_OUT_DPM
#undef MIDD_OUT_SLOTS_RULE

// What every out_conv launch refuses, and what it launches with: the dynamic LDS of (ic, C) and the 16x16 tiles of a sample
static bool out_conv_shape_ok(const OutConvArgs& a, size_t* lds, int* tiles) {
    if (a.ic > 4 || a.C % 16) return false;
    if (out_conv_lds_bytes(a.ic, a.C) > POINTWISE_LDS_LIMIT) return false;      // (refused at mi_unet_plan_create)
    *lds = out_conv_dynamic_lds_bytes(a.ic, a.C);
    *tiles = ((a.W + OC_T - 1) / OC_T) * ((a.H + OC_T - 1) / OC_T);
    return true;
}

// The arguments of an update that draws its noise term for virtual samples (a.seeded of launch_reference and launch_ddim)
static bool out_conv_seeded_ok(const OutConvArgs& a) {
    if ((unsigned long long)a.ic * a.H * a.W >= (1ull << 32) || a.members < 1 || a.v0 < 0) return false;
    if (a.tiles_x && (a.tiles_x < 1 || a.tiles_y < 1 || a.members != a.tiles_x * a.tiles_y || a.img_H < a.H || a.img_W < a.W ||
                      (unsigned long long)a.ic * a.img_H * a.img_W >= (1ull << 32))) return false;
    return true;
}

// KERNEL<1> for the grayscale case, KERNEL<0> otherwise, over a.B * tiles workgroups; the arguments follow
#define MIDD_OUT_LAUNCH(KERNEL, ...) \
    do { \
        if (a.ic == 1) hipLaunchKernelGGL(KERNEL<1>, dim3(a.B * tiles), dim3(256), lds, s, __VA_ARGS__); \
        else hipLaunchKernelGGL(KERNEL<0>, dim3(a.B * tiles), dim3(256), lds, s, __VA_ARGS__); \
    } while (0)

static hipError_t launch_reference(const OutConvArgs& a, hipStream_t s) {
    size_t lds; int tiles;
    if (!out_conv_shape_ok(a, &lds, &tiles)) return hipErrorInvalidValue;
    if (a.seeded) {
        if (!a.x || !out_conv_seeded_ok(a)) return hipErrorInvalidValue;
        MIDD_OUT_LAUNCH(out_conv_seeded_kernel, a, a.w);
    } else MIDD_OUT_LAUNCH(out_conv_kernel, a, a.w);
    return hipGetLastError();
}

// a.seeded != 0: the noise term of the slots with SLOT_NOISE is drawn from (a.seed, rec.image, rec.iter, element in the record's frame, rec.member); else it
// is read from a.noise when that is given.  a.c1 .. a.c3, a.iter, a.sample_offset, a.v0, a.members and the tile fields are not read.
static hipError_t launch_slots(const OutConvArgs& a, const SlotRec* slots, hipStream_t s) {
    size_t lds; int tiles;
    if (!out_conv_shape_ok(a, &lds, &tiles) || !slots || !a.x) return hipErrorInvalidValue;
    if (a.seeded && (a.noise || (unsigned long long)a.ic * a.H * a.W >= (1ull << 32))) return hipErrorInvalidValue;
    MIDD_OUT_LAUNCH(out_conv_slots_kernel, a, a.w, slots);
    return hipGetLastError();
}

// a.c1 .. a.c3 are not read.  The seeded form is launched only when a term is drawn at all (a.seeded: the host sets it with k.s > 0)
static hipError_t launch_ddim(const OutConvArgs& a, const DdimCoef& k, hipStream_t s) {
    size_t lds; int tiles;
    if (!out_conv_shape_ok(a, &lds, &tiles) || !a.x) return hipErrorInvalidValue;
    if (a.seeded) {
        if (a.noise || !out_conv_seeded_ok(a)) return hipErrorInvalidValue;
        MIDD_OUT_LAUNCH(out_conv_ddim_seeded_kernel, a, a.w, k);
    } else MIDD_OUT_LAUNCH(out_conv_ddim_kernel, a, a.w, k);
    return hipGetLastError();
}

// a.c1 .. a.c3, a.noise and the seeded fields are not read: the rule has no noise term.  x0_prev is read only when k.g != 0
static hipError_t launch_dpm(const OutConvArgs& a, const DpmCoef& k, const float* x0_prev, float* x0_out, hipStream_t s) {
    size_t lds; int tiles;
    if (!out_conv_shape_ok(a, &lds, &tiles) || !a.x || !x0_out || (k.g != 0.0f && !x0_prev)) return hipErrorInvalidValue;
    if (a.seeded || a.noise) return hipErrorInvalidValue;
    MIDD_OUT_LAUNCH(out_conv_dpm_kernel, a, a.w, k, x0_prev, x0_out);
    return hipGetLastError();
}

// The records' flags decide what a slot reads: x0_hist is null under the DDIM rule (no record has SLOT_HIST: the host), and the
// multistep rule has no noise term
static hipError_t launch_slots_rule(const OutConvArgs& a, const SlotRuleStep& u, hipStream_t s) {
    size_t lds; int tiles;
    if (!out_conv_shape_ok(a, &lds, &tiles) || !u.recs || !a.x) return hipErrorInvalidValue;
    if (a.seeded && (a.noise || (unsigned long long)a.ic * a.H * a.W >= (1ull << 32))) return hipErrorInvalidValue;
    if (u.x0_hist && (a.seeded || a.noise)) return hipErrorInvalidValue;
    MIDD_OUT_LAUNCH(out_conv_slots_rule_kernel, a, a.w, u.recs, u.clip_x0, u.x0_hist);
    return hipGetLastError();
}
#undef MIDD_OUT_LAUNCH

// The one launcher (midd_internal.h: OutUpdate) and, beside it, the symbol it launches: one switch each over the same kinds
hipError_t out_conv_launch(const OutConvArgs& a, const OutUpdate& u, hipStream_t s) {
    switch (u.kind) {
        case OUT_SLOTS: return launch_slots(a, u.slots, s);
        case OUT_SLOTS_RULE: return launch_slots_rule(a, u.slots_rule, s);
        case OUT_DDIM: return launch_ddim(a, u.ddim, s);
        case OUT_DPM: return launch_dpm(a, u.dpm.k, u.dpm.x0_prev, u.dpm.x0_out, s);
        case OUT_REFERENCE: {
            OutConvArgs r = a;
            r.c1 = u.ref.c1; r.c2 = u.ref.c2; r.c3 = u.ref.c3;
            return launch_reference(r, s);
        }
        case OUT_FORWARD: break;
    }
    return launch_reference(a, s);
}

const char* out_conv_symbol(const OutUpdate& u, int seeded) {
    switch (u.kind) {
        case OUT_SLOTS: return "out_conv_slots_kernel";
        case OUT_SLOTS_RULE: return "out_conv_slots_rule_kernel";
        case OUT_DDIM: return seeded ? "out_conv_ddim_seeded_kernel" : "out_conv_ddim_kernel";
        case OUT_DPM: return "out_conv_dpm_kernel";
        case OUT_REFERENCE: case OUT_FORWARD: break;
    }
    return seeded ? "out_conv_seeded_kernel" : "out_conv_kernel";
}

// One row of mi_denoise_slots for n <= SLOTS_PER_LAUNCH samples: their records travel as kernel arguments (copied when the launch
// is enqueued: nothing on the device ever reads the caller's host tables) into the program's record region, and every sample's
// time-table row into trow (0 for an idle slot: the network kernels still run over it).
__global__ void slot_fill_kernel(int* trow, SlotRec* dst, SlotRecs recs, int n) {
    if ((int)threadIdx.x < n) { trow[threadIdx.x] = recs.v[threadIdx.x].trow; dst[threadIdx.x] = recs.v[threadIdx.x]; }
}

hipError_t slot_fill_launch(int* trow, SlotRec* dst, const SlotRecs& recs, int n, hipStream_t s) {
    if (n < 1 || n > SLOTS_PER_LAUNCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(slot_fill_kernel, dim3(1), dim3(SLOTS_PER_LAUNCH), 0, s, trow, dst, recs, n);
    return hipGetLastError();
}

// the same for a row of mi_denoise_slots_rule: SlotRuleRec, 64 bytes a slot
__global__ void slot_rule_fill_kernel(int* trow, SlotRuleRec* dst, SlotRuleRecs recs, int n) {
    if ((int)threadIdx.x < n) { trow[threadIdx.x] = recs.v[threadIdx.x].trow; dst[threadIdx.x] = recs.v[threadIdx.x]; }
}

hipError_t slot_rule_fill_launch(int* trow, SlotRuleRec* dst, const SlotRuleRecs& recs, int n, hipStream_t s) {
    if (n < 1 || n > SLOTS_PER_LAUNCH) return hipErrorInvalidValue;
    hipLaunchKernelGGL(slot_rule_fill_kernel, dim3(1), dim3(SLOTS_PER_LAUNCH), 0, s, trow, dst, recs, n);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ seeded step noise as a tensor
// dst [n_iters][B][chw] <- step_noise_value(seed, sample_offset + b, iteration, element, member): what out_conv_seeded_kernel
// draws for the same (seed, image, iteration, element, member), so a seeded run -- or one member of an ensemble -- replays through
// mi_denoise's `step_noise`.  grid (chunks of 256 elements, B, n_iters)
__global__ __launch_bounds__(256)
void step_noise_fill_kernel(float* __restrict__ dst, unsigned long long chw, unsigned long long seed, long long sample_offset, unsigned member) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    if (e >= chw) return;
    const int b = blockIdx.y, it = blockIdx.z;
    dst[((size_t)it * gridDim.y + b) * chw + e] = step_noise_value(seed, sample_offset + b, it, (uint32_t)e, member);
}

hipError_t step_noise_fill_launch(float* dst, int n_iters, int B, unsigned long long chw, unsigned long long seed, long long sample_offset,
                                  unsigned member, hipStream_t s) {
    if (n_iters < 1 || B < 1 || chw < 1 || chw >= (1ull << 32) || n_iters > 65535 || B > 65535) return hipErrorInvalidValue;
    hipLaunchKernelGGL(step_noise_fill_kernel, dim3((unsigned)((chw + 255) / 256), B, n_iters), dim3(256), 0, s, dst, chw, seed, sample_offset, member);
    return hipGetLastError();
}

}  // namespace midd
