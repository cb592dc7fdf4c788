// The training objective as an evaluation call (include/midd.h: THE FORWARD NOISE, THE NOISING, THE DENOISING LOSS): the argument
// rules and the C ABI of mi_noise_images, mi_loss_terms and mi_denoising_loss.  The kernels are in diffusion_loss.hip.
//
// Reference code replaced:
//   DiffusionDenoiser.noise_images      Backend/DDIM/DDIMModel.py:259-263
//   the objective of the training loop  Backend/DDIM/DDIMModel.py:351-375, Backend/cddpm/cddpmModels.py:367-374
#include "midd_sampler.h"

using namespace midd;

namespace {

// The rules the three calls share (no GPU work) -> the per-sample records: a, s in fp32 in the reference's order, counter words c1, c2
int loss_records(const int32_t* t, const float* alpha_hat, int noise_steps, const void* eps, int seeded, int64_t sample_offset, int64_t draw,
                 const int64_t* sample_index, const int64_t* draws, int B, int C, int H, int W, std::vector<LossRec>* recs) {
    if (!t || !alpha_hat) return fail(MI_EINVAL, "null argument");
    if (B < 1 || C < 1 || H < 1 || W < 1) return fail(MI_EINVAL, "B, C, H and W must be positive, got (%d, %d, %d, %d)", B, C, H, W);
    if (C > 65535) return fail(MI_EINVAL, "C must be at most 65535, got %d", C);
    if (H > LOSS_MAX_SIDE || W > LOSS_MAX_SIDE) return fail(MI_EINVAL, "H and W must be at most 2^30, got (%d, %d)", H, W);
    if (noise_steps < 1) return fail(MI_EINVAL, "noise_steps must be positive, got %d", noise_steps);
    for (int b = 0; b < B; ++b)
        if (t[b] < 0 || t[b] >= noise_steps) return fail(MI_EINVAL, "timestep %d of sample %d outside [0, %d)", t[b], b, noise_steps);
    if (draw < 0 || draw >= (1LL << 31)) return fail(MI_EINVAL, "draw must be in [0, 2^31), got %lld", (long long)draw);
    if (sample_offset < 0) return fail(MI_EINVAL, "sample_offset must be >= 0, got %lld", (long long)sample_offset);
    for (int b = 0; b < B; ++b) {
        if (draws && (draws[b] < 0 || draws[b] >= (1LL << 31))) return fail(MI_EINVAL, "draw must be in [0, 2^31), got %lld for sample %d", (long long)draws[b], b);
        if (sample_index && sample_index[b] < 0) return fail(MI_EINVAL, "sample_index must be >= 0, got %lld for sample %d", (long long)sample_index[b], b);
    }
    if ((unsigned long long)C * H * W >= (1ull << 32)) return fail(MI_EINVAL, "C*H*W must stay below 2^32 (the element index is one 32-bit counter word)");
    if (seeded && eps) return fail(MI_EINVAL, "both a seed and eps: the noise is either drawn on the device or the caller's tensor");
    if (!seeded && !eps) return fail(MI_EINVAL, "neither a seed nor eps: the call needs a noise source");
    if (!seeded && (sample_index || draws)) return fail(MI_EINVAL, "sample_index or draws without a seed: they are the generator's counter words");
    recs->resize(B);
    for (int b = 0; b < B; ++b) {
        LossRec& r = (*recs)[b];
        r.a = sqrtf(alpha_hat[t[b]]);
        r.s = sqrtf(1.0f - alpha_hat[t[b]]);
        r.sample = (uint32_t)(uint64_t)(sample_index ? sample_index[b] : sample_offset + b);
        r.draw = (uint32_t)(draws ? draws[b] : draw);
    }
    return MI_OK;
}

bool word_aligned(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }

size_t round256(size_t n) { return (n + 255) & ~(size_t)255; }

}  // namespace

extern "C" int mi_noise_images(const float* clean, const int32_t* t, const float* alpha_hat, int noise_steps,
                               const float* eps, int seeded, uint64_t seed, int64_t sample_offset, int64_t draw,
                               const int64_t* sample_index, const int64_t* draws,
                               float* x_t, float* eps_out, int B, int C, int H, int W, void* stream) {
    if (!clean || !x_t) return fail(MI_EINVAL, "null argument");
    std::vector<LossRec> recs;
    if (const int rc = loss_records(t, alpha_hat, noise_steps, eps, seeded, sample_offset, draw, sample_index, draws, B, C, H, W, &recs)) return rc;
    if (!seeded && eps_out) return fail(MI_EINVAL, "eps_out with eps: the caller already holds the noise");
    if (!word_aligned(clean) || !word_aligned(x_t) || !word_aligned(eps) || !word_aligned(eps_out)) return fail(MI_EINVAL, "tensors must be 4-byte aligned");
    return launched(noise_images_launch(clean, eps, x_t, eps_out, recs.data(), B, (unsigned long long)C * H * W, seeded, seed,
                                        (hipStream_t)stream), "noise_images");
}

extern "C" size_t mi_loss_workspace_bytes(int B, int C, int H, int W) {
    if (B < 1 || C < 1 || C > 65535 || H < 1 || W < 1 || H > LOSS_MAX_SIDE || W > LOSS_MAX_SIDE || (unsigned long long)C * H * W >= (1ull << 32)) {
        fail(MI_EINVAL, "B, C, H and W must be positive, C <= 65535, H and W <= 2^30 and C*H*W below 2^32");
        return 0;
    }
    return round256(loss_partials_bytes(B, C, H, W));
}

extern "C" int mi_loss_terms(const float* clean, const float* x_t, const float* eps, const float* eps_pred,
                             const int32_t* t, const float* alpha_hat, int noise_steps,
                             int seeded, uint64_t seed, int64_t sample_offset, int64_t draw,
                             const int64_t* sample_index, const int64_t* draws, int flags, double edge_weight,
                             double* out, float* maps, int B, int C, int H, int W,
                             void* workspace, size_t workspace_bytes, void* stream) {
    if (!clean || !eps_pred || !out || !workspace) return fail(MI_EINVAL, "null argument");
    std::vector<LossRec> recs;
    if (const int rc = loss_records(t, alpha_hat, noise_steps, eps, seeded, sample_offset, draw, sample_index, draws, B, C, H, W, &recs)) return rc;
    if (seeded && x_t) return fail(MI_EINVAL, "both a seed and x_t: the seeded form makes x_t again from the seed");
    if (!seeded && !x_t) return fail(MI_EINVAL, "null argument: the explicit form reads x_t");
    if (!(edge_weight == edge_weight)) return fail(MI_EINVAL, "edge_weight is NaN");
    if (reinterpret_cast<uintptr_t>(workspace) & 7 || reinterpret_cast<uintptr_t>(out) & 7) return fail(MI_EINVAL, "workspace and out must be 8-byte aligned");
    if (!word_aligned(clean) || !word_aligned(x_t) || !word_aligned(eps) || !word_aligned(eps_pred) || !word_aligned(maps))
        return fail(MI_EINVAL, "tensors must be 4-byte aligned");
    if (workspace_bytes < loss_partials_bytes(B, C, H, W))
        return fail(MI_ENOMEM, "workspace too small: need %zu bytes, got %zu", loss_partials_bytes(B, C, H, W), workspace_bytes);
    return launched(loss_terms_launch(clean, x_t, eps, eps_pred, recs.data(), B, C, H, W, seeded, seed, flags & MI_CLAMP_EPS,
                                      edge_weight, out, maps, static_cast<double*>(workspace), (hipStream_t)stream), "loss_terms");
}

// workspace of mi_denoising_loss: [workspace of the forward's program | x_t [B,C,H,W] | eps_pred [B,C,H,W] | patch sums], each rounded up
// to 256 bytes.  The one description the size query and the call share
struct LossLayout { size_t xt_off, pred_off, part_off, bytes; };
static LossLayout loss_layout(const Program* g, int B, int C, int H, int W) {
    const size_t image = round256((size_t)B * C * H * W * sizeof(float));
    LossLayout l;
    l.xt_off = round256(g->bytes);
    l.pred_off = l.xt_off + image;
    l.part_off = l.pred_off + image;
    l.bytes = l.part_off + round256(loss_partials_bytes(B, C, H, W));
    return l;
}

extern "C" size_t mi_denoising_loss_workspace_bytes(mi_plan* plan, int B, int H, int W) {
    if (!plan) { fail(MI_EINVAL, "null plan"); return 0; }
    Program* g = nullptr;
    if (get_program(plan, B, H, W, &g)) return 0;      // (needs a finalized plan, as mi_workspace_bytes)
    return loss_layout(g, B, plan->cfg.in_channels, H, W).bytes;
}

extern "C" int mi_denoising_loss(mi_plan* plan, const float* clean, const float* cond, const int32_t* t,
                                 const float* alpha_hat, int noise_steps,
                                 const float* eps, int seeded, uint64_t seed, int64_t sample_offset, int64_t draw,
                                 const int64_t* sample_index, const int64_t* draws, int flags, double edge_weight,
                                 double* out, float* maps, int B, int H, int W,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (!clean || !cond || !out) return fail(MI_EINVAL, "null argument");
    const int C = plan->cfg.in_channels;
    std::vector<LossRec> recs;
    if (const int rc = loss_records(t, alpha_hat, noise_steps, eps, seeded, sample_offset, draw, sample_index, draws, B, C, H, W, &recs)) return rc;
    if (!(edge_weight == edge_weight)) return fail(MI_EINVAL, "edge_weight is NaN");
    if (reinterpret_cast<uintptr_t>(out) & 7) return fail(MI_EINVAL, "out must be 8-byte aligned");
    if (!word_aligned(clean) || !word_aligned(eps) || !word_aligned(maps)) return fail(MI_EINVAL, "tensors must be 4-byte aligned");
    Program* g = nullptr;
    if (const int rc = get_program(plan, B, H, W, &g)) return rc;
    const LossLayout lay = loss_layout(g, B, C, H, W);
    if (const int rc = check_workspace(workspace, workspace_bytes, lay.bytes)) return rc;
    if (const int rc = check_finalized(plan)) return rc;
    if (const int rc = check_device(plan)) return rc;
    for (int b = 0; b < B; ++b)
        if (t[b] >= plan->time_rows) return fail(MI_EINVAL, "timestep %d outside the precomputed table [0,%d)", t[b], plan->time_rows);

    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* x_t = reinterpret_cast<float*>(ws + lay.xt_off);
    float* pred = reinterpret_cast<float*>(ws + lay.pred_off);
    const unsigned long long chw = (unsigned long long)C * H * W;
    HIPCHK(hipMemsetAsync(ws, 0, 256, s));                  // status word
    int rc = launched(noise_images_launch(clean, eps, x_t, nullptr, recs.data(), B, chw, seeded, seed, s), "noise_images");
    if (rc) return rc;
    if ((rc = launched(fill_i32_launch(reinterpret_cast<int*>(ws + g->trow_off), t, B, s), "fill timesteps"))) return rc;
    StepIO io{};
    io.x = x_t; io.cond = cond; io.eps_out = pred;
    if ((rc = run_program(plan, g, io, ws, reinterpret_cast<int*>(ws), s))) return rc;
    // seeded: the loss kernel forms z and x_t again (x_t in the workspace fed the network only); explicit: it reads both
    return launched(loss_terms_launch(clean, seeded ? nullptr : x_t, eps, pred, recs.data(), B, C, H, W, seeded, seed,
                                      flags & MI_CLAMP_EPS, edge_weight, out, maps, reinterpret_cast<double*>(ws + lay.part_off), s), "loss_terms");
}
