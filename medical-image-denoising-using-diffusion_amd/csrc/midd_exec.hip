// Executor: walks a Program's launch list (mi_unet_forward), the sampler loop (mi_denoise), debug fetch and per-op profiling.
#include "midd_host.h"
#include "tile_geometry.h"

using namespace midd;

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
// and the update rule of the uniform calls (include/midd.h: mi_update_rule; ddim == 0: the reference's)
struct Schedule {
    const int32_t* t; int n; const float *beta, *alpha, *alpha_hat; int noise_steps;
    int ddim = 0; double eta = 0.0; int clip_x0 = 1;
    // dpm != 0 (include/midd.h: THE DPMPP2M UPDATE; ddim stays 0): the caller's history of predicted images, one run's worth
    // [slots][B, C, H, W] -- x0_stride 0: one slot, read and written in place; else the elements between two slots of the trajectory
    int dpm = 0; float* x0 = nullptr; size_t x0_stride = 0;
};

struct StepIO {
    const float* x; const float* cond; float* eps_out;
    float* x_update; const float* noise; float c1, c2, c3; int clamp_eps;
    // ddim != 0: the update is the DDIM(eta) rule with this row of the coefficient table (out_conv_ddim_launch); c1 .. c3 are not read
    int ddim; DdimCoef coef;
    // dpm != 0: the second-order multistep rule instead (out_conv_dpm_launch): its row, the previous predicted image (read when
    // dcoef.g != 0) and where this iteration's is written; of the fields above the update reads x_update and clamp_eps only
    int dpm; DpmCoef dcoef; const float* x0_prev; float* x0_out;
    // sn.seeded: the update draws its noise term (step_noise_common.h) for iteration `iter`, sample 0 of THIS program being virtual
    // sample sn.v0; a step that draws nothing keeps the defaults (sn.tensor is not read: `noise` is this step's slice of it)
    int iter; StepNoise sn;
    // slots != null (mi_denoise_slots): every sample is updated from its record of this row (device, [B]) by out_conv_slots_kernel;
    // of the fields above the update reads x_update, noise, clamp_eps, sn.seeded and sn.seed only
    const SlotRec* slots;
};

// the rc of a launch wrapper's hipError_t
static int launched(hipError_t e, const char* what) {
    return e == hipSuccess ? MI_OK : fail(MI_EHIP, "%s: %s", what, hipGetErrorString(e));
}

// status: the call's status word (first word of the CALLER's workspace, whichever sub-batch program runs)
static int run_program(mi_plan* p, Program* g, const StepIO& io, char* ws, int* status, hipStream_t s,
                       hipEvent_t mid_event = nullptr, int mid_div = 2) {
    const float* wd = p->wdev;
    auto F = [&](size_t off) { return reinterpret_cast<float*>(ws + off); };
    const int B = g->B;
    auto T = [&](size_t off) { return reinterpret_cast<stat_word*>(ws + off); };
    // every tensor's GroupNorm totals start the forward at zero (producers accumulate with atomics)
    if (hipMemsetAsync(ws + g->stats_off, 0, g->stats_bytes, s) != hipSuccess) return fail(MI_EHIP, "clearing the statistics arena failed");
    // split-fp16 plans keep their activations channel-blocked, [B][C/16][H][W][16] (midd_internal.h); fp32-MFMA plans NHWC
    const int blocked = fp16_mfma(p->cfg) ? 1 : 0;
    const int planes = operand_planes(p->cfg);
    for (const Op& o : g->ops) {
        hipError_t e = hipSuccess;
        hipEvent_t ev_a = nullptr, ev_b = nullptr;
        if (p->profiling) {
            auto take = [&]() -> hipEvent_t {
                hipEvent_t ev = nullptr;
                if (!p->event_pool.empty()) { ev = p->event_pool.back(); p->event_pool.pop_back(); }
                else if (hipEventCreate(&ev) != hipSuccess) ev = nullptr;
                return ev;
            };
            ev_a = take(); ev_b = take();
            if (!ev_a || !ev_b) return fail(MI_EHIP, "hipEventCreate failed");
            (void)hipEventRecord(ev_a, s);
        }
        switch (o.kind) {
            case OP_IN_CONV:
                e = in_conv_launch(io.x, io.cond, wd + p->w_in, wd + p->b_in, F(o.dst.off), T(o.dst.tot_off), g->stat_rep, o.dst.stat_bs,
                                   B, p->cfg.in_channels, g->H, g->W, o.dst.C, blocked, s);
                break;
            case OP_CHAN_TOT:
                e = chan_total_launch(F(o.s0.off), T(o.s0.tot_off), g->stat_rep, o.s0.stat_bs, B, o.s0.H * o.s0.W, o.s0.C, o.stat_rows, blocked, s);
                break;
            case OP_CONV: {
                ConvArgs a{};
                a.src0 = F(o.s0.off); a.C0 = o.s0.C;
                a.src1 = o.has_s1 ? F(o.s1.off) : nullptr; a.C1 = o.has_s1 ? o.s1.C : 0;
                a.B = B; a.H = o.s0.H; a.W = o.s0.W; a.OH = o.dst.H; a.OW = o.dst.W;
                a.wpack = wd + o.w; a.bias = wd + o.b; a.Cout = o.dst.C;
                a.prologue = o.prologue; a.stat_rep = g->stat_rep;
                a.raw_scale_fixed = o.raw_scale_fixed; a.status = status;
                if (o.res_steps > 0) {
                    a.res_steps = o.res_steps; a.res_scale = o.res_scale;
                    a.res_src0 = F(o.res0.off); a.res_C0 = o.res0.C;
                    a.res_src1 = o.has_res1 ? F(o.res1.off) : nullptr; a.res_C1 = o.has_res1 ? o.res1.C : 0;
                    if (o.res0.stat_id >= 0 && (!o.has_res1 || o.res1.stat_id >= 0)) {
                        a.res_tot0 = T(o.res0.tot_off); a.res_bs0 = o.res0.stat_bs;
                        a.res_tot1 = o.has_res1 ? T(o.res1.tot_off) : T(o.res0.tot_off); a.res_bs1 = o.has_res1 ? o.res1.stat_bs : 1;
                    }
                }
                if (o.att_mode != ATT_NONE) {
                    const Att16Layout lay = attention16_layout(B, o.dst.H * o.dst.W, o.att_mode == ATT_QKV_OUT ? o.dst.C / 3 : o.dst.C, planes);
                    a.att_mode = o.att_mode; a.att_heads = ATTN_HEADS_ABI; a.att_D = (o.att_mode == ATT_QKV_OUT ? o.dst.C / 3 : o.dst.C) / ATTN_HEADS_ABI;
                    a.att_npad = lay.npad; a.att_ksplit = o.att_ksplit;
                    a.att_k = reinterpret_cast<_Float16*>(ws + o.partial_off + lay.k_off); a.att_v = reinterpret_cast<_Float16*>(ws + o.partial_off + lay.v_off);
                    a.att_ml = reinterpret_cast<const float*>(ws + o.partial_off + lay.ml_off);
                }
                if (o.gn.on || o.raw_stats) {
                    a.gn_tot0 = T(o.s0.tot_off); a.gn_bs0 = o.s0.stat_bs;
                    a.gn_tot1 = o.has_s1 ? T(o.s1.tot_off) : T(o.s0.tot_off); a.gn_bs1 = o.has_s1 ? o.s1.stat_bs : 1;
                }
                if (o.gn.on) {
                    a.gn_gamma = wd + o.gn.gamma; a.gn_beta = wd + o.gn.beta; a.gn_eps = 1e-5f;
                    a.gn_inv_n = 1.0 / ((double)o.s0.H * o.s0.W * ((a.C0 + a.C1) / GN_GROUPS_));
                }
                if (o.temb_col >= 0) { a.temb = p->ttab + o.temb_col; a.temb_stride = p->temb_cols; a.trow = reinterpret_cast<const int*>(ws + g->trow_off); }
                a.resid = o.has_resid ? F(o.resid.off) : nullptr;
                a.out = F(o.dst.off); a.out_scale = o.out_scale;
                if (o.want_stats) { a.stat_tot = T(o.dst.tot_off); a.stat_bs = o.dst.stat_bs; }
                a.persist_wgs = g->persist_wgs;
                e = fp16_mfma(p->cfg) ? conv16_launch(a, o.tile, s) : conv_launch(a, o.tile, s);      // (the tile carries the planes)
                break;
            }
            case OP_ATTN:
                if (fp16_mfma(p->cfg)) {
                    const int N = o.dst.H * o.dst.W, C = o.dst.C;
                    const Att16Layout lay = attention16_layout(B, N, C, planes);
                    char* sc = ws + o.partial_off;
                    e = attention16_launch(F(o.s0.off), reinterpret_cast<const _Float16*>(sc + lay.k_off), reinterpret_cast<const _Float16*>(sc + lay.v_off),
                                           reinterpret_cast<float*>(sc + lay.po_off), reinterpret_cast<float*>(sc + lay.ml_off),
                                           B, o.att_ksplit, o.att_tps, N, C, ATTN_HEADS_ABI, s, planes);
                } else {
                    e = attention_launch(F(o.s0.off), F(o.dst.off), B, o.dst.H * o.dst.W, o.dst.C, 2, s);
                }
                break;
            case OP_RESIZE:
                e = resize_bilinear_launch(F(o.s0.off), F(o.dst.off), T(o.dst.tot_off), g->stat_rep, o.dst.stat_bs, B, o.s0.H, o.s0.W, o.s0.C, o.dst.H, o.dst.W, blocked, s);
                break;
            case OP_CONVT:
                e = conv_transpose_launch(F(o.s0.off), wd + o.w, wd + o.b, F(o.dst.off), B, o.s0.H, o.s0.W, o.s0.C, o.dst.C, blocked, s);
                break;
            case OP_OUT: {
                OutConvArgs a{};
                a.src = F(o.s0.off); a.blocked = blocked; a.gn_tot = T(o.s0.tot_off); a.stat_rep = g->stat_rep; a.gn_bs = o.s0.stat_bs; a.gn_gamma = wd + o.gn.gamma; a.gn_beta = wd + o.gn.beta; a.gn_eps = 1e-5f;
                a.w = wd + p->w_out; a.bias = wd + p->b_out;
                a.B = B; a.H = g->H; a.W = g->W; a.C = o.s0.C; a.ic = p->cfg.in_channels;
                a.eps_out = io.eps_out; a.x = io.x_update; a.noise = io.noise;
                a.c1 = io.c1; a.c2 = io.c2; a.c3 = io.c3; a.clamp_eps = io.clamp_eps;
                const StepNoise& n = io.sn;
                a.seeded = n.seeded; a.iter = io.iter; a.seed = n.seed; a.sample_offset = n.sample_offset;
                a.v0 = n.v0; a.members = n.members > 0 ? n.members : 1; a.member_offset = n.member_offset;
                a.tiles_x = n.tiles_x; a.tiles_y = n.tiles_y; a.img_H = n.img_H; a.img_W = n.img_W;
                e = io.slots ? out_conv_slots_launch(a, io.slots, s) : io.ddim ? out_conv_ddim_launch(a, io.coef, s)
                  : io.dpm ? out_conv_dpm_launch(a, io.dcoef, io.x0_prev, io.x0_out, s) : out_conv_launch(a, s);
                break;
            }
        }
        if (e != hipSuccess) return fail(MI_EHIP, "kernel launch (op kind %d) failed: %s", (int)o.kind, hipGetErrorString(e));
        // phase offset of the next sub-batch: it starts when this one has passed 1/(2 parts) of its ops -- a quarter of a forward
        // for two sub-batches (same-box sweep of 25 / 35 / 50 / 65 / 75 %: 46.4 / 46.1 / 45.7 / 45.9 / 45.9 images/s; round 2 used 50 %)
        const size_t mid_at = g->ops.size() / (2 * (size_t)mid_div);
        if (mid_event && (size_t)(&o - g->ops.data()) == mid_at) (void)hipEventRecord(mid_event, s);
        if (p->profiling) {
            (void)hipEventRecord(ev_b, s);
            mi_plan::Span sp; sp.a = ev_a; sp.b = ev_b;
            op_work(p, g, o, &sp.name, &sp.flops, &sp.bytes);
            const size_t oc_at = sp.name.find("out_conv_kernel");
            if (o.kind == OP_OUT && (io.sn.seeded || io.slots || io.ddim || io.dpm) && oc_at != std::string::npos)      // the symbol that ran
                sp.name.replace(oc_at, 15, io.slots ? "out_conv_slots_kernel" : io.ddim ? (io.sn.seeded ? "out_conv_ddim_seeded_kernel" : "out_conv_ddim_kernel")
                                                                             : io.dpm ? "out_conv_dpm_kernel" : "out_conv_seeded_kernel");
            static const bool per_op = getenv("MIDD_PROFILE_PER_OP") != nullptr;      // one entry per op instead of per symbol
            if (per_op) {
                char tag[96];
                snprintf(tag, sizeof(tag), "op%03d %dx%d c%d+%d->%d k%d s%d | ", (int)(&o - g->ops.data()), o.dst.H, o.dst.W,
                         o.s0.C, o.has_s1 ? o.s1.C : 0, o.dst.C, o.ks, o.stride);
                sp.name = std::string(tag) + sp.name;
            }
            p->spans.push_back(std::move(sp));
        }
    }
    return MI_OK;
}

static int check_device(mi_plan* plan) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != plan->device)
        return fail(MI_ESTATE, "plan was finalized on device %d but current device is %d", plan->device, dev);
    return MI_OK;
}

static int check_finalized(mi_plan* plan) {
    return plan->finalized ? MI_OK : fail(MI_ESTATE, "mi_unet_finalize has not been called (or weights changed since)");
}

static int check_workspace(const void* ws, size_t got, size_t need) {
    if (!ws || got < need) return fail(MI_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, got);
    if (((uintptr_t)ws) & 255) return fail(MI_EINVAL, "workspace must be 256-byte aligned");
    return MI_OK;
}

static int check_call(mi_plan* plan, int B, int H, int W, void* ws, size_t ws_bytes, Program** g) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (int rc = get_program(plan, B, H, W, g)) return rc;
    if (int rc = check_workspace(ws, ws_bytes, (*g)->bytes)) return rc;
    return check_device(plan);
}

// every entry of a timestep list indexes the schedule's tables (check_schedule, check_ddim)
static int check_t_list(const int32_t* t, int n, int noise_steps) {
    for (int i = 0; i < n; ++i)
        if (t[i] < 0 || t[i] >= noise_steps) return fail(MI_EINVAL, "t_list[%d]=%d outside [0,%d)", i, t[i], noise_steps);
    return MI_OK;
}

// the sampler's host-side arguments (mi_denoise*, and the batched calls before their first pass)
static int check_schedule(mi_plan* plan, const Schedule& sc) {
    if ((sc.n > 0 && !sc.t) || !sc.beta || !sc.alpha || !sc.alpha_hat) return fail(MI_EINVAL, "null argument");
    if (sc.n < 0 || sc.noise_steps < 1 || sc.noise_steps > plan->time_rows)
        return fail(MI_EINVAL, "noise_steps %d exceeds the precomputed time table (%d rows)", sc.noise_steps, plan->time_rows);
    return check_t_list(sc.t, sc.n, sc.noise_steps);
}

// THE DDIM UPDATE, host side (include/midd.h): row i of the coefficient table of a list, in double precision from the caller's
// fp32 table, every value rounded once to fp32.  A = alpha_hat[t_i], P = alpha_hat[t_{i+1}], 1 after the last entry.  The one
// place that computes it: mi_ddim_coefficients exports it, enqueue_run passes its rows to the update kernel.
static void ddim_row(const int32_t* t, int n, const float* alpha_hat, double eta, int i, float out[7]) {
#pragma clang fp contract(off)
    const double A = (double)alpha_hat[t[i]], P = i + 1 < n ? (double)alpha_hat[t[i + 1]] : 1.0;
    const double sigma = eta * std::sqrt((1.0 - P) / (1.0 - A)) * std::sqrt(1.0 - A / P);
    const double rest = (1.0 - P) - sigma * sigma;
    out[0] = (float)(1.0 / std::sqrt(A)); out[1] = (float)std::sqrt(1.0 - A); out[2] = (float)std::sqrt(A); out[3] = (float)(1.0 / std::sqrt(1.0 - A));
    out[4] = (float)std::sqrt(P); out[5] = (float)std::sqrt(rest > 0.0 ? rest : 0.0); out[6] = (float)(2.0 * sigma);
}

// the rule's own argument rules, host only and before anything else of a call: eta, the list, the table entries the list reads
static int check_ddim(const int32_t* t, int n, const float* alpha_hat, int noise_steps, double eta) {
    if (!(eta >= 0.0 && eta <= 1.0)) return fail(MI_EINVAL, "eta %.17g outside [0, 1] (limit: 0 <= eta <= 1, not NaN)", eta);
    if (n < 0 || (n > 0 && !t) || !alpha_hat) return fail(MI_EINVAL, "null argument");
    if (noise_steps < 1) return fail(MI_EINVAL, "noise_steps %d: a schedule has at least one step (limit: noise_steps >= 1)", noise_steps);
    if (int rc = check_t_list(t, n, noise_steps)) return rc;
    for (int i = 1; i < n; ++i) {
        if (t[i] >= t[i - 1])
            return fail(MI_EINVAL, "t_list[%d]=%d after t_list[%d]=%d: the DDIM update jumps from each timestep to the next one of the list "
                        "(limit: a strictly decreasing list)", i, t[i], i - 1, t[i - 1]);
    }
    for (int i = 0; i < n; ++i) {
        const double A = (double)alpha_hat[t[i]], P = i + 1 < n ? (double)alpha_hat[t[i + 1]] : 1.0;
        if (!(A > 0.0 && A < P && P <= 1.0))
            return fail(MI_EINVAL, "alpha_hat[%d]=%.9g, next %.9g: the DDIM update needs 0 < alpha_hat[t_i] < alpha_hat[t_{i+1}] <= 1", t[i], A, P);
    }
    return MI_OK;
}

extern "C" int mi_ddim_coefficients(const int32_t* t_list, int n_iters, const float* alpha_hat, int noise_steps, double eta, float* out) {
    if (int rc = check_ddim(t_list, n_iters, alpha_hat, noise_steps, eta)) return rc;
    if (n_iters > 0 && !out) return fail(MI_EINVAL, "null argument");
    for (int i = 0; i < n_iters; ++i) ddim_row(t_list, n_iters, alpha_hat, eta, i, out + (size_t)i * 7);
    return MI_OK;
}

// THE DPMPP2M UPDATE, host side (include/midd.h): the multistep weight of row i, in double precision from the caller's fp32 table,
// every operation rounded on its own, rounded once to fp32.  0 on the first row (no history) and on the last (P = 1, h infinite).
// The one place that computes it: mi_dpm_coefficients exports it, enqueue_run passes it to the update kernel.
static double dpm_lambda(double X) {
#pragma clang fp contract(off)
    return 0.5 * std::log(X / (1.0 - X));
}
static float dpm_g(const int32_t* t, int n, const float* alpha_hat, int i) {
#pragma clang fp contract(off)
    if (i < 1 || i + 1 >= n) return 0.0f;
    const double Q = (double)alpha_hat[t[i - 1]], A = (double)alpha_hat[t[i]], P = (double)alpha_hat[t[i + 1]];
    const double lA = dpm_lambda(A);
    const double h = dpm_lambda(P) - lA, h_prev = lA - dpm_lambda(Q);
    const double r = h_prev / h;
    const double emh = std::sqrt(((1.0 - P) / (1.0 - A)) * (A / P));      // e^{-h} without exp
    // the extrapolation weight 1 / (2 r) bounded at its uniform-step value 1/2 (why)
    return (float)(std::sqrt(P) * (1.0 - emh) / (2.0 * (r > 1.0 ? r : 1.0)));
}

extern "C" int mi_dpm_coefficients(const int32_t* t_list, int n_iters, const float* alpha_hat, int noise_steps, float* out) {
    if (int rc = check_ddim(t_list, n_iters, alpha_hat, noise_steps, 0.0)) return rc;
    if (n_iters > 0 && !out) return fail(MI_EINVAL, "null argument");
    for (int i = 0; i < n_iters; ++i) {
        ddim_row(t_list, n_iters, alpha_hat, 0.0, i, out + (size_t)i * 8);
        out[(size_t)i * 8 + 7] = dpm_g(t_list, n_iters, alpha_hat, i);
    }
    return MI_OK;
}

// A call's rule -> its Schedule.  NULL or kind MI_UPDATE_REFERENCE: the schedule stays the reference's.  Judged first in every
// *_rule call, so a bad rule or list is MI_EINVAL whatever the plan's state.
static int apply_rule(const mi_update_rule* rule, Schedule* sc) {
    if (!rule || rule->kind == MI_UPDATE_REFERENCE) return MI_OK;
    if (rule->kind == MI_UPDATE_DPMPP2M)
        return fail(MI_EINVAL, "update rule MI_UPDATE_DPMPP2M needs a buffer for the predicted images, which this call does not take: "
                    "call mi_denoise_dpm or mi_denoise_tiled_dpm");
    if (rule->kind != MI_UPDATE_DDIM) return fail(MI_EINVAL, "unknown update rule %d (MI_UPDATE_REFERENCE or MI_UPDATE_DDIM)", (int)rule->kind);
    if (int rc = check_ddim(sc->t, sc->n, sc->alpha_hat, sc->noise_steps, rule->eta)) return rc;
    sc->ddim = 1; sc->eta = rule->eta; sc->clip_x0 = rule->clip_x0 ? 1 : 0;
    return MI_OK;
}

// no two of the n buffers may overlap (a null one is absent); `why` is the call's sentence on who reads and who writes
struct Buf { const void* p; size_t bytes; const char* name; };
static int check_no_overlap(const Buf* b, int n, const char* why) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const uintptr_t a = (uintptr_t)b[i].p, c = (uintptr_t)b[j].p;
            if (a && c && a < c + b[j].bytes && c < a + b[i].bytes)
                return fail(MI_EINVAL, "%s and %s alias (overlap): %s", b[i].name, b[j].name, why);
        }
    return MI_OK;
}

extern "C" int mi_unet_forward(mi_plan* plan, const float* x, const float* condition, const int32_t* t, float* eps,
                               int B, int H, int W, void* workspace, size_t workspace_bytes, void* stream) {
    Program* g = nullptr;
    int rc = check_call(plan, B, H, W, workspace, workspace_bytes, &g);
    if (rc) return rc;
    if (!x || !condition || !t || !eps) return fail(MI_EINVAL, "null argument");
    for (int i = 0; i < B; ++i)
        if (t[i] < 0 || t[i] >= plan->time_rows) return fail(MI_EINVAL, "timestep %d outside the precomputed table [0,%d)", t[i], plan->time_rows);
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    HIPCHK(hipMemsetAsync(ws, 0, 256, s));                  // status word
    if ((rc = launched(fill_i32_launch(reinterpret_cast<int*>(ws + g->trow_off), t, B, s), "fill timesteps"))) return rc;
    StepIO io{};
    io.x = x; io.cond = condition; io.eps_out = eps;
    return run_program(plan, g, io, ws, reinterpret_cast<int*>(ws), s);
}

// One batch through the sampler loop, in two steps: check_run judges the arguments (no GPU work), enqueue_run enqueues the
// batch.  enqueue_run neither takes the plan's side-stream mutex nor clears the status word: its caller does both, once per
// C call -- denoise_run for mi_denoise / mi_denoise_seeded, a batched call once for all its passes (run_passes), so that the
// word accumulates over them.
static int check_run(mi_plan* plan, const float* noisy, const float* x_out, int B, int H, int W, const Schedule& sc,
                     void* workspace, size_t workspace_bytes, Program** g) {
    int rc = check_call(plan, B, H, W, workspace, workspace_bytes, g);
    if (rc) return rc;
    if (!noisy || !x_out) return fail(MI_EINVAL, "null argument");
    if ((rc = check_schedule(plan, sc))) return rc;
    if (noisy == x_out) return fail(MI_EINVAL, "x_out must not alias noisy (the condition image is read every step)");
    return MI_OK;
}

// The rows of a sampler call.  Uniform (mi_denoise and its siblings, slots == null): row i puts every sample at sc.t[i], x starts
// as a copy of the condition images.  Slots (mi_denoise_slots): sc.t is a table [n][B], sample b is at t[i * B + b] in row i or
// idle (-1), its noise counter words are (sample_index[b], iter_base[b] + i), and x is the caller's: it is not initialised.
struct SlotRows {
    const int32_t* iter_base;         // [B] or null (all 0)
    const int64_t* sample_index;      // [B] or null (0 .. B-1)
};

// (the caller holds plan->side_mu and has cleared the status word at the head of `workspace`)
static int enqueue_run(mi_plan* plan, Program* g, const float* noisy, float* x_out, int B, int H, int W,
                       const Schedule& sc, const SlotRows* slots, const StepNoise& sn, int flags,
                       void* workspace, size_t workspace_bytes, void* stream) {
    const int n_iters = sc.n;
    const float *beta = sc.beta, *alpha = sc.alpha, *alpha_hat = sc.alpha_hat;
    int rc = MI_OK;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const size_t img_elems = (size_t)B * plan->cfg.in_channels * H * W;
    if (!slots) HIPCHK(hipMemcpyAsync(x_out, noisy, img_elems * sizeof(float), hipMemcpyDeviceToDevice, s));   // x = noisy_img.clone()
    // Images are independent: the batch runs as `parts` sub-batches on as many streams, each started
    // 1/parts of a forward after the previous one, so that one part's latency-bound low-resolution
    // layers (one workgroup per CU at B=8) share the chip with another part's HBM-bound high-resolution
    // layers.  parts == 1: the whole-batch program on the caller's stream, no side stream, no event.
    const int parts = ((flags & MI_NO_SPLIT) || n_iters == 0) ? 1 : split_parts(B);
    Program* gh = g;
    if (parts > 1) {
        if ((rc = get_program(plan, B / parts, H, W, &gh, true))) return rc;
        if (workspace_bytes < parts * gh->bytes) return fail(MI_ENOMEM, "workspace too small for the split run: need %zu bytes", parts * gh->bytes);
        if (!plan->sev_fork) HIPCHK(hipEventCreateWithFlags(&plan->sev_fork, hipEventDisableTiming));
        for (int h = 1; h < parts; ++h) {
            if (!plan->sstream[h]) {
                // The side stream runs at high queue priority (-1): its workgroups are dispatched
                // ahead of the caller's stream whenever both have work ready, which keeps the two
                // half-batch programs out of phase.  Same-box sweep, 256x256 B=16: priority 0
                // 46.0 img/s, -1 46.7, +1 46.0.  MIDD_SIDE_PRIO overrides (development knob).
                static const int side_prio = getenv("MIDD_SIDE_PRIO") ? atoi(getenv("MIDD_SIDE_PRIO")) : -1;
                HIPCHK(hipStreamCreateWithPriority(&plan->sstream[h], hipStreamNonBlocking, side_prio));
                HIPCHK(hipEventCreateWithFlags(&plan->sev_join[h], hipEventDisableTiming));
            }
            if (!plan->sev_phase[h - 1]) HIPCHK(hipEventCreateWithFlags(&plan->sev_phase[h - 1], hipEventDisableTiming));
        }
        HIPCHK(hipEventRecord(plan->sev_fork, s));
        for (int h = 1; h < parts; ++h) HIPCHK(hipStreamWaitEvent(plan->sstream[h], plan->sev_fork, 0));
    }
    const size_t part = img_elems / parts;
    // From here on the side streams may hold work on x_out and the workspace: whatever happens in the loop,
    // the caller's stream waits for them before this call returns (the caller frees / reuses both).
    auto enqueue_all = [&]() -> int {
        const int Bh = B / parts;
        for (int i = 0; i < n_iters; ++i) {
            for (int h = 0; h < parts; ++h) {
                hipStream_t sh = h ? plan->sstream[h] : s;
                char* wsh = ws + (size_t)h * gh->bytes;
                StepIO io{};
                io.x = x_out + h * part; io.cond = noisy + h * part; io.eps_out = nullptr; io.x_update = x_out + h * part;
                // fp32 arithmetic in the reference's order (DDIMModel.py:280-283)
                auto coeffs = [&](int t, float* c1, float* c2, float* c3) {
                    *c1 = 1.0f / sqrtf(alpha[t]);
                    *c2 = (1.0f - alpha[t]) / sqrtf(1.0f - alpha_hat[t]);
                    *c3 = sqrtf(beta[t]);
                };
                if (slots) {
                    // sub-batch h takes columns [h * Bh, (h + 1) * Bh) of every table; the records leave as kernel arguments
                    int* trow = reinterpret_cast<int*>(wsh + gh->trow_off);
                    SlotRec* recs = reinterpret_cast<SlotRec*>(wsh + gh->slot_off);
                    for (int c0 = 0; c0 < Bh; c0 += SLOTS_PER_LAUNCH) {
                        SlotRecs r{};
                        const int m = Bh - c0 < SLOTS_PER_LAUNCH ? Bh - c0 : SLOTS_PER_LAUNCH;
                        for (int j = 0; j < m; ++j) {
                            const int col = h * Bh + c0 + j, t = sc.t[(size_t)i * B + col];
                            if (t < 0) continue;                             // idle: active 0, time row 0
                            SlotRec& q = r.v[j];
                            coeffs(t, &q.c1, &q.c2, &q.c3);
                            q.active = SLOT_ACTIVE | ((t > 0 && (sn.seeded || sn.tensor)) ? SLOT_NOISE : 0);      // nothing is drawn at t == 0
                            q.iter = (unsigned)((slots->iter_base ? slots->iter_base[col] : 0) + i);
                            q.image = (unsigned)(uint64_t)(slots->sample_index ? slots->sample_index[col] : (int64_t)col);
                            q.trow = t;
                        }
                        if (int rc2 = launched(slot_fill_launch(trow + c0, recs + c0, r, m, sh), "slot records")) return rc2;
                    }
                    io.slots = recs;
                    io.noise = sn.tensor ? sn.tensor + (size_t)i * img_elems + h * part : nullptr;
                    io.sn.seeded = sn.seeded; io.sn.seed = sn.seed;
                } else {
                    const int t = sc.t[i];
                    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)(wsh + gh->trow_off), t, Bh, sh));          // t = full((B,), i)
                    bool draws = t > 0;                              // nothing is drawn at t == 0
                    if (sc.ddim) {
                        float r[7];
                        ddim_row(sc.t, n_iters, alpha_hat, sc.eta, i, r);
                        io.ddim = 1;
                        io.coef = DdimCoef{r[0], r[1], r[2], r[3], r[4], r[5], r[6], sc.clip_x0, i == n_iters - 1 ? 1 : 0};
                        draws = r[6] > 0.0f;                         // nor at s == 0: every row at eta == 0, always the last one
                    } else if (sc.dpm) {
                        float r[7];
                        ddim_row(sc.t, n_iters, alpha_hat, 0.0, i, r);
                        io.dpm = 1;
                        io.dcoef = DpmCoef{r[0], r[1], r[2], r[3], r[4], r[5], dpm_g(sc.t, n_iters, alpha_hat, i), sc.clip_x0, i == n_iters - 1 ? 1 : 0};
                        // iteration i reads slot i - 1 and writes slot i (in place when there is one slot); sub-batch h: its images
                        io.x0_out = sc.x0 + (size_t)i * sc.x0_stride + h * part;
                        io.x0_prev = i > 0 ? sc.x0 + (size_t)(i - 1) * sc.x0_stride + h * part : io.x0_out;      // (i == 0: g == 0, not read)
                        draws = false;                               // deterministic: no noise term
                    } else {
                        coeffs(t, &io.c1, &io.c2, &io.c3);
                    }
                    io.noise = (sn.tensor && draws) ? sn.tensor + (size_t)i * img_elems + h * part : nullptr;      // cddpmModels.py:297-300
                    if (sn.seeded && draws) {
                        io.iter = i; io.sn = sn;
                        io.sn.v0 += h * Bh;                          // sub-batch h: its first virtual index
                    }
                }
                io.clamp_eps = (flags & MI_CLAMP_EPS) ? 1 : 0;
                if (i == 0 && h > 0) HIPCHK(hipStreamWaitEvent(sh, plan->sev_phase[h - 1], 0));      // phase offset (re-establishing it every n-th
                                                                                                      // iteration measured -2 %: round 4; the streams run freely)
                hipEvent_t mid = (i == 0 && h + 1 < parts) ? plan->sev_phase[h] : nullptr;
                int rc2 = run_program(plan, gh, io, wsh, reinterpret_cast<int*>(ws), sh, mid, parts);
                if (rc2) return rc2;
            }
        }
        return MI_OK;
    };
    rc = enqueue_all();
    for (int h = 1; h < parts; ++h) {
        const hipError_t e1 = hipEventRecord(plan->sev_join[h], plan->sstream[h]);
        const hipError_t e2 = (e1 == hipSuccess) ? hipStreamWaitEvent(s, plan->sev_join[h], 0) : e1;
        if (e2 != hipSuccess) {                                   // cannot order the streams: drain the side stream
            (void)hipStreamSynchronize(plan->sstream[h]);
            if (rc == MI_OK) rc = fail(MI_EHIP, "joining side stream %d failed: %s", h, hipGetErrorString(e2));
        }
    }
    return rc;
}

// a sampler call of its own: arguments, the plan's side-stream mutex, the status word, the batch
static int denoise_run(mi_plan* plan, const float* noisy, float* x_out, int B, int H, int W, const Schedule& sc,
                       const StepNoise& sn, int flags, void* workspace, size_t workspace_bytes, void* stream) {
    Program* g = nullptr;
    if (int rc = check_run(plan, noisy, x_out, B, H, W, sc, workspace, workspace_bytes, &g)) return rc;
    std::lock_guard<std::mutex> side_lk(plan->side_mu);      // the side streams and their events are per plan: one enqueue at a time
    HIPCHK(hipMemsetAsync(workspace, 0, 256, (hipStream_t)stream));      // status word (before the side streams fork)
    return enqueue_run(plan, g, noisy, x_out, B, H, W, sc, nullptr, sn, flags, workspace, workspace_bytes, stream);
}

extern "C" int mi_denoise(mi_plan* plan, const float* noisy, float* x_out, int B, int H, int W,
                          const int32_t* t_list, int n_iters,
                          const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                          const float* step_noise, int flags,
                          void* workspace, size_t workspace_bytes, void* stream) {
    StepNoise sn;
    sn.tensor = step_noise;
    return denoise_run(plan, noisy, x_out, B, H, W, Schedule{t_list, n_iters, beta, alpha, alpha_hat, noise_steps}, sn, flags,
                       workspace, workspace_bytes, stream);
}

// the generator's counter words: element index and sample index (step_noise_common.h)
static int check_step_noise_range(int64_t C, int64_t H, int64_t W, int64_t sample_offset) {
    if (sample_offset < 0) return fail(MI_EINVAL, "sample_offset %lld is negative: the global sample index starts at 0", (long long)sample_offset);
    if (C < 1 || H < 1 || W < 1) return fail(MI_EINVAL, "bad image shape %lldx%lldx%lld", (long long)C, (long long)H, (long long)W);
    // (three factors below 2^31 each: the product of two fits 64 bits, the third is compared by division)
    if (C * H > (int64_t)0xFFFFFFFFll / W)
        return fail(MI_EINVAL, "C*H*W = %lld*%lld*%lld reaches 2^32: the element index of the seeded step noise is one 32-bit counter word "
                    "(limit: C*H*W < 4294967296)", (long long)C, (long long)H, (long long)W);
    return MI_OK;
}

extern "C" int mi_denoise_seeded(mi_plan* plan, const float* noisy, float* x_out, int B, int H, int W,
                                 const int32_t* t_list, int n_iters,
                                 const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                 uint64_t seed, int64_t sample_offset, int flags,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (int rc = check_step_noise_range(plan->cfg.in_channels, H, W, sample_offset)) return rc;
    StepNoise sn;
    sn.seeded = true; sn.seed = seed; sn.sample_offset = sample_offset;
    return denoise_run(plan, noisy, x_out, B, H, W, Schedule{t_list, n_iters, beta, alpha, alpha_hat, noise_steps}, sn, flags,
                       workspace, workspace_bytes, stream);
}

// mi_denoise and mi_denoise_seeded in one signature, with an update rule (NULL: the reference's, i.e. those two calls)
extern "C" int mi_denoise_rule(mi_plan* plan, const float* noisy, float* x_out, int B, int H, int W,
                               const int32_t* t_list, int n_iters,
                               const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                               const float* step_noise, int seeded, uint64_t seed, int64_t sample_offset, int flags,
                               const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream) {
    Schedule sc{t_list, n_iters, beta, alpha, alpha_hat, noise_steps};
    if (int rc = apply_rule(rule, &sc)) return rc;
    StepNoise sn;
    if (seeded) {
        if (step_noise) return fail(MI_EINVAL, "seeded together with step_noise: the noise term is drawn or read, not both");
        if (!plan) return fail(MI_EINVAL, "null plan");      // (as mi_denoise_seeded: the counter range needs the plan; unseeded, check_call answers)
        if (int rc = check_step_noise_range(plan->cfg.in_channels, H, W, sample_offset)) return rc;
        sn.seeded = true; sn.seed = seed; sn.sample_offset = sample_offset;
    } else {
        sn.tensor = step_noise;
    }
    return denoise_run(plan, noisy, x_out, B, H, W, sc, sn, flags, workspace, workspace_bytes, stream);
}

// The second-order multistep rule (include/midd.h: THE DPMPP2M UPDATE): mi_denoise plus the caller's buffer of predicted images
extern "C" int mi_denoise_dpm(mi_plan* plan, const float* noisy, float* x_out, float* x0_buf, int x0_slots, int B, int H, int W,
                              const int32_t* t_list, int n_iters,
                              const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                              int flags, int clip_x0, void* workspace, size_t workspace_bytes, void* stream) {
    Schedule sc{t_list, n_iters, beta, alpha, alpha_hat, noise_steps};
    if (int rc = check_ddim(t_list, n_iters, alpha_hat, noise_steps, 0.0)) return rc;      // the rule's own cases first, as mi_denoise_rule
    if (x0_slots != 1 && x0_slots != n_iters)
        return fail(MI_EINVAL, "x0_slots %d: 1 (the history in place) or n_iters = %d (the trajectory of predicted images)", x0_slots, n_iters);
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (n_iters > 0 && !x0_buf) return fail(MI_EINVAL, "null argument");
    if (B < 1 || H < 1 || W < 1) return fail(MI_EINVAL, "bad image shape %dx%dx%d", B, H, W);
    const size_t img_elems = (size_t)B * plan->cfg.in_channels * H * W;
    const Buf buf[3] = {{noisy, img_elems * sizeof(float), "noisy"}, {x_out, img_elems * sizeof(float), "x_out"},
                        {x0_buf, (size_t)x0_slots * img_elems * sizeof(float), "x0_buf"}};
    if (int rc = check_no_overlap(buf, 3, "noisy is read every step and x0_buf is written beside x_out")) return rc;
    sc.dpm = 1; sc.clip_x0 = clip_x0 ? 1 : 0; sc.x0 = x0_buf; sc.x0_stride = x0_slots > 1 ? img_elems : 0;
    return denoise_run(plan, noisy, x_out, B, H, W, sc, StepNoise{}, flags, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------- per-slot timesteps (continuous batching)
extern "C" int mi_denoise_slots(mi_plan* plan, const float* cond, float* x, int B, int H, int W,
                                const int32_t* t_rows, int n_rows, const int32_t* iter_base, const int64_t* sample_index,
                                const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                const float* step_noise, int seeded, uint64_t seed, int flags,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (!cond || !x || !beta || !alpha || !alpha_hat || (n_rows > 0 && !t_rows)) return fail(MI_EINVAL, "null argument");
    if (n_rows < 0) return fail(MI_EINVAL, "n_rows %d is negative (limit: n_rows >= 0)", n_rows);
    if (B < 1 || H < 1 || W < 1) return fail(MI_EINVAL, "bad shape B %d, %dx%d (limit: B >= 1, H >= 1, W >= 1)", B, H, W);
    if (noise_steps < 1) return fail(MI_EINVAL, "noise_steps %d: a schedule has at least one step (limit: noise_steps >= 1)", noise_steps);
    for (int b = 0; b < B; ++b) {
        bool idle = false;                                       // within a call a slot is active on a prefix of the rows
        for (int i = 0; i < n_rows; ++i) {
            const int t = t_rows[(size_t)i * B + b];
            if (t < -1 || t >= noise_steps)
                return fail(MI_EINVAL, "t_rows[%d][%d]=%d outside [-1,%d) (-1 = idle)", i, b, t, noise_steps);
            if (t >= 0 && idle)
                return fail(MI_EINVAL, "t_rows[%d][%d]=%d: slot %d is active again after an idle row (limit: a slot is active on a prefix "
                            "of the rows; a new image joins at the next call)", i, b, t, b);
            idle = t < 0;
        }
        if (iter_base && (iter_base[b] < 0 || (int64_t)iter_base[b] + n_rows > 2147483647ll))
            return fail(MI_EINVAL, "iter_base[%d]=%d with %d rows: the iteration index is one 32-bit counter word, kept below 2^31 "
                        "(limit: 0 <= iter_base, iter_base + n_rows <= 2147483647)", b, iter_base[b], n_rows);
        if (sample_index && sample_index[b] < 0)
            return fail(MI_EINVAL, "sample_index[%d]=%lld is negative: the global sample index starts at 0", b, (long long)sample_index[b]);
    }
    if (seeded) {
        if (step_noise) return fail(MI_EINVAL, "seeded together with step_noise: the noise term is drawn or read, not both");
        if (int rc = check_step_noise_range(plan->cfg.in_channels, H, W, 0)) return rc;
    }
    const size_t batch_bytes = (size_t)B * plan->cfg.in_channels * H * W * sizeof(float);
    const Buf buf[2] = {{x, batch_bytes, "x"}, {cond, batch_bytes, "cond"}};
    if (int rc = check_no_overlap(buf, 2, "the condition images are read by every row while x is updated in place")) return rc;
    if (int rc = check_finalized(plan)) return rc;
    if (noise_steps > plan->time_rows)
        return fail(MI_EINVAL, "noise_steps %d exceeds the precomputed time table (%d rows)", noise_steps, plan->time_rows);
    Program* g = nullptr;
    if (int rc = check_call(plan, B, H, W, workspace, workspace_bytes, &g)) return rc;
    if (n_rows == 0) return MI_OK;
    StepNoise sn;
    sn.tensor = step_noise; sn.seeded = seeded != 0; sn.seed = seed;
    const SlotRows slots{iter_base, sample_index};
    std::lock_guard<std::mutex> side_lk(plan->side_mu);
    HIPCHK(hipMemsetAsync(workspace, 0, 256, (hipStream_t)stream));      // status word: once per call
    return enqueue_run(plan, g, cond, x, B, H, W, Schedule{t_rows, n_rows, beta, alpha, alpha_hat, noise_steps}, &slots, sn, flags,
                       workspace, workspace_bytes, stream);
}

extern "C" int mi_step_noise_fill_member(float* dst, int n_iters, int B, int C, int H, int W,
                                         uint64_t seed, int64_t sample_offset, int64_t member, void* stream) {
    if (int rc = check_step_noise_range(C, H, W, sample_offset)) return rc;
    if (member < 0 || member >= ((int64_t)1 << 32))
        return fail(MI_EINVAL, "member %lld outside [0, 2^32): the member index is one 32-bit counter word (limit: member < 4294967296)", (long long)member);
    if (n_iters < 0 || B < 0 || n_iters > 65535 || B > 65535) return fail(MI_EINVAL, "n_iters %d / B %d outside [0, 65535]", n_iters, B);
    if (n_iters == 0 || B == 0) return MI_OK;
    if (!dst) return fail(MI_EINVAL, "null argument");
    return launched(step_noise_fill_launch(dst, n_iters, B, (unsigned long long)C * H * W, seed, sample_offset, (uint32_t)member, (hipStream_t)stream),
                    "step_noise_fill");
}

extern "C" int mi_step_noise_fill(float* dst, int n_iters, int B, int C, int H, int W,
                                  uint64_t seed, int64_t sample_offset, void* stream) {
    return mi_step_noise_fill_member(dst, n_iters, B, C, H, W, seed, sample_offset, 0, stream);
}

// ---------------------------------------------------------------------------- ensembles of the stochastic sampler
constexpr int64_t MEMBER_WORDS = (int64_t)1 << 32;      // the member index is one 32-bit counter word

static int check_members_min(int members) {
    return members >= 1 ? MI_OK : fail(MI_EINVAL, "members %d: an ensemble has at least one member (limit: members >= 1)", members);
}

static int check_std_members(const float* std_out, int members) {
    if (std_out && members < 2) return fail(MI_EINVAL, "std_out needs members >= 2: the unbiased standard deviation of one value is undefined");
    return MI_OK;
}

// B is grid.y of the reduce kernel
static int check_reduce_batch(int B, const char* why = "limit of the reduce kernel's grid") {
    return (B >= 1 && B <= 65535) ? MI_OK : fail(MI_EINVAL, "B %d outside [1, 65535] (%s)", B, why);
}

static int check_members(int members, int64_t member_offset) {
    if (int rc = check_members_min(members)) return rc;
    if (member_offset < 0) return fail(MI_EINVAL, "member_offset %lld is negative: member indices start at 0", (long long)member_offset);
    if (member_offset > MEMBER_WORDS - members)
        return fail(MI_EINVAL, "member_offset %lld + members %d exceeds 2^32: the member index of the seeded step noise is one 32-bit "
                    "counter word (limit: member_offset + members <= 4294967296)", (long long)member_offset, members);
    return MI_OK;
}

// B images x members draws: what the reduce kernel's grid (B in grid.y) and the 32-bit virtual index can hold
static int check_ensemble_size(int B, int members) {
    if (int rc = check_reduce_batch(B)) return rc;
    if ((int64_t)B * members > 2147483647ll)
        return fail(MI_EINVAL, "B * members = %d * %d exceeds 2^31 - 1: the virtual sample index is a 32-bit int (limit: B * members <= 2147483647)", B, members);
    return MI_OK;
}

int midd::check_ensemble_args(mi_plan* plan, int B, int members, int H, int W, int64_t sample_offset, int64_t member_offset, int pass_samples) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (int rc = check_members(members, member_offset)) return rc;
    if (pass_samples < 1) return fail(MI_EINVAL, "pass_samples %d: a pass holds at least one virtual sample (limit: pass_samples >= 1)", pass_samples);
    if (int rc = check_ensemble_size(B, members)) return rc;
    return check_step_noise_range(plan->cfg.in_channels, H, W, sample_offset);
}

extern "C" int mi_ensemble_reduce(const float* samples, int B, int members, int64_t chw, float* mean_out, float* std_out, void* stream) {
    if (int rc = check_members_min(members)) return rc;
    if (int rc = check_reduce_batch(B)) return rc;
    if (chw < 1 || chw >= MEMBER_WORDS) return fail(MI_EINVAL, "chw %lld outside [1, 2^32) (limit: C*H*W < 4294967296)", (long long)chw);
    if (int rc = check_std_members(std_out, members)) return rc;
    if (!samples || !mean_out) return fail(MI_EINVAL, "null argument");
    return launched(ensemble_reduce_launch(samples, B, members, (unsigned long long)chw, mean_out, std_out, (hipStream_t)stream), "ensemble_reduce");
}

// the members of a pixel are sorted in registers (ensemble.hip: ensemble_quantiles_kernel): at most QUANTILE_MAX_MEMBERS of them
static int check_quantile_members(int members) {
    if (members > QUANTILE_MAX_MEMBERS)
        return fail(MI_EINVAL, "members %d: the quantile kernels sort a pixel's members in registers (limit: members <= %d; mean and std have no such limit)",
                    members, QUANTILE_MAX_MEMBERS);
    return MI_OK;
}

// the levels of a quantile call, host doubles -> the kernel argument
static int check_quantile_levels(const double* q, int nq, QuantileLevels* ql) {
    if (nq < 1 || nq > QUANTILE_MAX_LEVELS)
        return fail(MI_EINVAL, "nq %d outside [1, %d]: the levels travel as kernel arguments (limit: 1 <= nq <= %d)", nq, QUANTILE_MAX_LEVELS, QUANTILE_MAX_LEVELS);
    if (!q) return fail(MI_EINVAL, "null argument");
    *ql = QuantileLevels{};
    ql->nq = nq;
    for (int i = 0; i < nq; ++i) {
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(MI_EINVAL, "q[%d] = %.17g outside [0, 1] (limit: 0 <= q <= 1, not NaN)", i, q[i]);
        ql->q[i] = q[i];
    }
    return MI_OK;
}

extern "C" int mi_ensemble_quantiles(const float* samples, int B, int members, int64_t chw, const double* q, int nq, float* out, void* stream) {
    if (int rc = check_members_min(members)) return rc;
    if (int rc = check_reduce_batch(B)) return rc;
    if (chw < 1 || chw >= MEMBER_WORDS) return fail(MI_EINVAL, "chw %lld outside [1, 2^32) (limit: C*H*W < 4294967296)", (long long)chw);
    if (int rc = check_quantile_members(members)) return rc;
    QuantileLevels ql;
    if (int rc = check_quantile_levels(q, nq, &ql)) return rc;
    if (!samples || !out) return fail(MI_EINVAL, "null argument");
    return launched(ensemble_quantiles_launch(samples, B, members, (unsigned long long)chw, ql, out, (hipStream_t)stream), "ensemble_quantiles");
}

// ---------------------------------------------------------------------------- the batched calls: virtual samples in passes
// mi_denoise_ensemble, mi_denoise_tiled and mi_denoise_tiled_ensemble run `rounds` x V virtual samples of h x w each through the
// sampler loop in passes of L.pass.  Each judges its own argument rules and its table of buffers (check_no_overlap), then shares
// check_batched_call and run_passes, and ends with its own reduce / blend launch.

// What lies between a batched call's own rules and its first launch, in the order in which it is reported: the plan's state, the
// workspace layout (the caller's ensemble_layout / tiled_ensemble_layout call: its rc and result), the workspace's size and
// alignment, the pointers that must not be null, the schedule -- what a pass would refuse is refused here, before anything is
// enqueued -- and the device.
static int check_batched_call(mi_plan* plan, int layout_rc, const EnsembleLayout& L, const void* ws, size_t ws_bytes,
                              std::initializer_list<const void*> required, const Schedule& sc) {
    if (int rc = check_finalized(plan)) return rc;
    if (layout_rc) return layout_rc;                     // (mi_last_error holds the planner's message)
    if (int rc = check_workspace(ws, ws_bytes, L.bytes)) return rc;
    for (const void* p : required)
        if (!p) return fail(MI_EINVAL, "null argument");
    if (int rc = check_schedule(plan, sc)) return rc;
    return check_device(plan);
}

// The one pass loop.  Round m (a member of the tiled ensemble, whose member word is a launch constant; else the only round) runs
// the virtual samples [0, V) in passes: fill(cond, v0, n) writes the pass's condition images, the sampler loop leaves its
// samples at store[m][v0 ..].  The caller holds plan->side_mu and has cleared the status word, so the word accumulates over the
// passes; every pass joins its side streams before it returns, on success and on failure (enqueue_run), and the first failing
// pass ends the call.
template <class Fill>
static int run_passes(mi_plan* plan, Fill fill, float* store, int64_t V, int rounds, int h, int w, size_t chw, const EnsembleLayout& L,
                      StepNoise sn, const Schedule& sc, int flags, char* ws, void* stream) {
    float* cond = reinterpret_cast<float*>(ws + L.cond_off);
    const uint32_t member_base = sn.member_offset;
    for (int m = 0; m < rounds; ++m) {
        sn.member_offset = member_base + m;
        for (int64_t v0 = 0; v0 < V; v0 += L.pass) {
            const int n = (int)(V - v0 < L.pass ? V - v0 : L.pass);
            if (int rc = fill(cond, (int)v0, n)) return rc;
            sn.v0 = (int)v0;
            Program* g = nullptr;
            float* x = store + ((size_t)m * V + (size_t)v0) * chw;
            if (int rc = check_run(plan, cond, x, n, h, w, sc, ws, L.run_bytes, &g)) return rc;
            if (int rc = enqueue_run(plan, g, cond, x, n, h, w, sc, nullptr, sn, flags, ws, L.run_bytes, stream)) return rc;
        }
    }
    return MI_OK;
}

extern "C" int mi_denoise_ensemble_rule(mi_plan* plan, const float* noisy, float* mean_out, float* std_out, float* samples_out,
                                        int B, int members, int H, int W,
                                        const int32_t* t_list, int n_iters,
                                        const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                        uint64_t seed, int64_t sample_offset, int64_t member_offset, int pass_samples, int flags,
                                        const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream) {
    Schedule sc{t_list, n_iters, beta, alpha, alpha_hat, noise_steps};
    if (int rc = apply_rule(rule, &sc)) return rc;
    if (int rc = check_ensemble_args(plan, B, members, H, W, sample_offset, member_offset, pass_samples)) return rc;
    if (!mean_out && !std_out && !samples_out) return fail(MI_EINVAL, "no output: give at least one of mean_out, std_out, samples_out");
    if (int rc = check_std_members(std_out, members)) return rc;
    const size_t chw = (size_t)plan->cfg.in_channels * H * W, img = chw * sizeof(float);
    const Buf buf[4] = {{noisy, (size_t)B * img, "noisy"}, {mean_out, (size_t)B * img, "mean_out"}, {std_out, (size_t)B * img, "std_out"},
                        {samples_out, (size_t)B * members * img, "samples_out"}};
    if (int rc = check_no_overlap(buf, 4, "noisy is read every step and the reduce reads samples_out while it writes mean_out and std_out"))
        return rc;
    EnsembleLayout L{};
    // (evaluated before the state check, reported after it: check_batched_call; host arithmetic only, as in the *_workspace_bytes queries)
    const int layout_rc = ensemble_layout(plan, B, members, H, W, pass_samples, samples_out != nullptr, &L);
    if (int rc = check_batched_call(plan, layout_rc, L, workspace, workspace_bytes, {noisy}, sc)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* samples = samples_out ? samples_out : reinterpret_cast<float*>(ws + L.samples_off);
    std::lock_guard<std::mutex> side_lk(plan->side_mu);     // held over all passes: the side streams are per plan
    HIPCHK(hipMemsetAsync(ws, 0, 256, s));                  // status word: once per call, the passes accumulate into it
    StepNoise sn;
    sn.seeded = true; sn.seed = seed; sn.sample_offset = sample_offset; sn.members = members; sn.member_offset = (uint32_t)member_offset;
    auto broadcast = [&](float* cond, int v0, int n) { return launched(ensemble_broadcast_launch(noisy, cond, v0, n, members, chw, s), "ensemble_broadcast"); };
    if (int rc = run_passes(plan, broadcast, samples, (int64_t)B * members, 1, H, W, chw, L, sn, sc, flags, ws, stream)) return rc;
    if (mean_out || std_out) return launched(ensemble_reduce_launch(samples, B, members, chw, mean_out, std_out, s), "ensemble_reduce");
    return MI_OK;
}

extern "C" int mi_denoise_ensemble(mi_plan* plan, const float* noisy, float* mean_out, float* std_out, float* samples_out,
                                   int B, int members, int H, int W,
                                   const int32_t* t_list, int n_iters,
                                   const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                   uint64_t seed, int64_t sample_offset, int64_t member_offset, int pass_samples, int flags,
                                   void* workspace, size_t workspace_bytes, void* stream) {
    return mi_denoise_ensemble_rule(plan, noisy, mean_out, std_out, samples_out, B, members, H, W, t_list, n_iters, beta, alpha, alpha_hat,
                                    noise_steps, seed, sample_offset, member_offset, pass_samples, flags, nullptr, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------- tiled denoising of full-resolution images
static int check_tile_axis(const char* axis, int L, int T, int O) {
    if (T < 1) return fail(MI_EINVAL, "tile %s %d must be positive", axis, T);
    if (T > L) return fail(MI_EINVAL, "tile %s %d exceeds the image %s %d (limit: tile <= image; resize a smaller image up, or use a smaller tile)", axis, T, axis, L);
    if (O < 0 || O > T / 2) return fail(MI_EINVAL, "overlap %d of tile %s %d outside [0, %d] (limit: 0 <= overlap <= tile / 2)", O, axis, T, T / 2);
    return MI_OK;
}

extern "C" int mi_tile_geometry(int L, int T, int O, int* n, int* origins, int cap) {
    if (int rc = check_tile_axis("length", L, T, O)) return rc;
    if (!n) return fail(MI_EINVAL, "null argument");
    *n = tile_count(L, T, O);
    for (int i = 0; origins && i < *n && i < cap; ++i) origins[i] = tile_origin(i, L, T, *n);
    return MI_OK;
}

static int fill_tile_geom(int C, int H, int W, int th, int tw, int oy, int ox, TileGeom* g) {
    if (int rc = check_tile_axis("height", H, th, oy)) return rc;
    if (int rc = check_tile_axis("width", W, tw, ox)) return rc;
    if (oy > 46339 || ox > 46339) return fail(MI_EINVAL, "overlap %dx%d: the window product must fit 32 bits (limit: overlap <= 46339)", oy, ox);
    *g = TileGeom{C, H, W, th, tw, oy, ox, tile_count(H, th, oy), tile_count(W, tw, ox)};
    return MI_OK;
}

static int check_tile_count(int B, const TileGeom& g) {
    if (B < 1) return fail(MI_EINVAL, "B %d must be positive", B);
    if ((int64_t)B * g.ny * g.nx > 2147483647ll)
        return fail(MI_EINVAL, "B * tiles = %d * %d * %d exceeds 2^31 - 1: the virtual sample index is a 32-bit int (limit: B * tiles <= 2147483647)", B, g.ny, g.nx);
    return MI_OK;
}

int midd::check_tiled_args(mi_plan* plan, int B, int H, int W, int th, int tw, int oy, int ox, int64_t sample_offset, int pass_samples, TileGeom* g) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    const int div = 1 << (plan->levels - 1);
    if (th < div || tw < div || th % div || tw % div)
        return fail(MI_EINVAL, "tile %dx%d: the network takes positive multiples of %d only (limit of the plan; the IMAGE may have any size >= the tile)", th, tw, div);
    if (int rc = fill_tile_geom(plan->cfg.in_channels, H, W, th, tw, oy, ox, g)) return rc;
    if (pass_samples < 1) return fail(MI_EINVAL, "pass_samples %d: a pass holds at least one tile (limit: pass_samples >= 1)", pass_samples);
    if (int rc = check_step_noise_range(plan->cfg.in_channels, H, W, sample_offset)) return rc;
    return check_tile_count(B, *g);
}

extern "C" int mi_tile_extract(const float* noisy, int B, int C, int H, int W, int th, int tw, int oy, int ox, int v0, int n,
                               float* dst, void* stream) {
    TileGeom g{};
    if (C < 1) return fail(MI_EINVAL, "C %d must be positive", C);
    if (int rc = fill_tile_geom(C, H, W, th, tw, oy, ox, &g)) return rc;
    if (int rc = check_tile_count(B, g)) return rc;
    if (v0 < 0 || n < 0 || n > 65535 || (int64_t)v0 + n > (int64_t)B * g.ny * g.nx)
        return fail(MI_EINVAL, "tiles [%d, %d + %d) outside the %d * %d * %d tiles of the batch (limit per call: n <= 65535)", v0, v0, n, B, g.ny, g.nx);
    if ((int64_t)C * th * tw > 2147483647ll) return fail(MI_EINVAL, "C*th*tw = %d*%d*%d exceeds 2^31 - 1", C, th, tw);
    if (n == 0) return MI_OK;
    if (!noisy || !dst) return fail(MI_EINVAL, "null argument");
    return launched(tile_extract_launch(noisy, dst, g, v0, n, (hipStream_t)stream), "tile_extract");
}

extern "C" int mi_tile_blend(const float* tiles, int B, int C, int H, int W, int th, int tw, int oy, int ox, float* out, void* stream) {
    TileGeom g{};
    if (C < 1) return fail(MI_EINVAL, "C %d must be positive", C);
    if (int rc = fill_tile_geom(C, H, W, th, tw, oy, ox, &g)) return rc;
    if (int rc = check_tile_count(B, g)) return rc;
    if (int rc = check_step_noise_range(C, H, W, 0)) return rc;
    if (!tiles || !out) return fail(MI_EINVAL, "null argument");
    return launched(tile_blend_launch(tiles, out, B, g, (hipStream_t)stream), "tile_blend");
}

// mi_denoise_tiled_rule and mi_denoise_tiled_dpm behind their rules: `sc` carries the rule.  sc.dpm: sc.x0 is the call's x0_hist
// [pass_samples, C, th, tw], the in-place history of whichever pass runs
static int tiled_run(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out,
                     int B, int H, int W, int th, int tw, int oy, int ox, const Schedule& sc,
                     int seeded, uint64_t seed, int64_t sample_offset, int pass_samples, int flags,
                     void* workspace, size_t workspace_bytes, void* stream) {
    TileGeom tg{};
    if (int rc = check_tiled_args(plan, B, H, W, th, tw, oy, ox, sample_offset, pass_samples, &tg)) return rc;
    const int K = tg.ny * tg.nx;
    const size_t chw = (size_t)tg.C * th * tw, img = (size_t)tg.C * H * W * sizeof(float);
    if (sc.dpm && sc.n > 0 && !sc.x0) return fail(MI_EINVAL, "null argument");
    const Buf buf[4] = {{noisy, (size_t)B * img, "noisy"}, {image_out, (size_t)B * img, "image_out"},
                        {tiles_out, (size_t)B * K * chw * sizeof(float), "tiles_out"},
                        {sc.dpm ? sc.x0 : nullptr, (size_t)pass_samples * chw * sizeof(float), "x0_hist"}};
    if (int rc = check_no_overlap(buf, 4, "noisy is read by every pass and the blend reads the tiles while it writes image_out")) return rc;
    EnsembleLayout L{};
    // (evaluated before the state check, reported after it: check_batched_call; host arithmetic only, as in the *_workspace_bytes queries)
    const int layout_rc = ensemble_layout(plan, B, K, th, tw, pass_samples, tiles_out != nullptr, &L);
    if (int rc = check_batched_call(plan, layout_rc, L, workspace, workspace_bytes, {noisy, image_out}, sc)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* tiles = tiles_out ? tiles_out : reinterpret_cast<float*>(ws + L.samples_off);
    std::lock_guard<std::mutex> side_lk(plan->side_mu);     // held over all passes: the side streams are per plan
    HIPCHK(hipMemsetAsync(ws, 0, 256, s));                  // status word: once per call, the passes accumulate into it
    StepNoise sn;
    if (seeded) {
        sn.seeded = true; sn.seed = seed; sn.sample_offset = sample_offset; sn.members = K;
        sn.tiles_x = tg.nx; sn.tiles_y = tg.ny; sn.img_H = H; sn.img_W = W;
    }
    auto extract = [&](float* cond, int v0, int n) { return launched(tile_extract_launch(noisy, cond, tg, v0, n, s), "tile_extract"); };
    if (int rc = run_passes(plan, extract, tiles, (int64_t)B * K, 1, th, tw, chw, L, sn, sc, flags, ws, stream)) return rc;
    return launched(tile_blend_launch(tiles, image_out, B, tg, s), "tile_blend");
}

extern "C" int mi_denoise_tiled_rule(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out,
                                     int B, int H, int W, int th, int tw, int oy, int ox,
                                     const int32_t* t_list, int n_iters,
                                     const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                     int seeded, uint64_t seed, int64_t sample_offset, int pass_samples, int flags,
                                     const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream) {
    Schedule sc{t_list, n_iters, beta, alpha, alpha_hat, noise_steps};
    if (int rc = apply_rule(rule, &sc)) return rc;
    return tiled_run(plan, noisy, image_out, tiles_out, B, H, W, th, tw, oy, ox, sc, seeded, seed, sample_offset, pass_samples, flags,
                     workspace, workspace_bytes, stream);
}

// mi_denoise_tiled under the second-order multistep rule: deterministic, so no seed; the history of a pass lives in x0_hist
extern "C" int mi_denoise_tiled_dpm(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out, float* x0_hist,
                                    int B, int H, int W, int th, int tw, int oy, int ox,
                                    const int32_t* t_list, int n_iters,
                                    const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                    int pass_samples, int flags, int clip_x0, void* workspace, size_t workspace_bytes, void* stream) {
    Schedule sc{t_list, n_iters, beta, alpha, alpha_hat, noise_steps};
    if (int rc = check_ddim(t_list, n_iters, alpha_hat, noise_steps, 0.0)) return rc;
    if (n_iters > 0 && !x0_hist) return fail(MI_EINVAL, "null argument");
    sc.dpm = 1; sc.clip_x0 = clip_x0 ? 1 : 0; sc.x0 = x0_hist; sc.x0_stride = 0;
    return tiled_run(plan, noisy, image_out, tiles_out, B, H, W, th, tw, oy, ox, sc, 0, 0, 0, pass_samples, flags,
                     workspace, workspace_bytes, stream);
}

extern "C" int mi_denoise_tiled(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out,
                                int B, int H, int W, int th, int tw, int oy, int ox,
                                const int32_t* t_list, int n_iters,
                                const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                int seeded, uint64_t seed, int64_t sample_offset, int pass_samples, int flags,
                                void* workspace, size_t workspace_bytes, void* stream) {
    return mi_denoise_tiled_rule(plan, noisy, image_out, tiles_out, B, H, W, th, tw, oy, ox, t_list, n_iters, beta, alpha, alpha_hat, noise_steps,
                                 seeded, seed, sample_offset, pass_samples, flags, nullptr, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------- ensembles of tiled runs
// members x B images x tiles: the tile storage is indexed by a 32-bit int (check_tile_count has judged B * tiles)
static int check_tiled_ensemble_size(int B, int members, const TileGeom& g) {
    if ((int64_t)B * g.ny * g.nx * members > 2147483647ll)
        return fail(MI_EINVAL, "B * members * tiles = %d * %d * %d * %d exceeds 2^31 - 1: the tile index of the member storage is a 32-bit int "
                    "(limit: B * members * tiles <= 2147483647)", B, members, g.ny, g.nx);
    return MI_OK;
}

int midd::check_tiled_ensemble_args(mi_plan* plan, int B, int members, int H, int W, int th, int tw, int oy, int ox,
                                    int64_t sample_offset, int64_t member_offset, int pass_samples, TileGeom* g) {
    if (int rc = check_tiled_args(plan, B, H, W, th, tw, oy, ox, sample_offset, pass_samples, g)) return rc;
    if (int rc = check_members(members, member_offset)) return rc;
    return check_tiled_ensemble_size(B, members, *g);
}

extern "C" int mi_tile_blend_reduce(const float* tiles, int B, int members, int C, int H, int W, int th, int tw, int oy, int ox,
                                    float* mean_out, float* std_out, float* samples_out, void* stream) {
    TileGeom g{};
    if (C < 1) return fail(MI_EINVAL, "C %d must be positive", C);
    if (int rc = fill_tile_geom(C, H, W, th, tw, oy, ox, &g)) return rc;
    if (int rc = check_tile_count(B, g)) return rc;
    if (int rc = check_step_noise_range(C, H, W, 0)) return rc;
    if (int rc = check_members_min(members)) return rc;
    if (int rc = check_reduce_batch(B, "the limit of mi_ensemble_reduce, whose arithmetic this call composes")) return rc;      // (B >= 1: check_tile_count)
    if (int rc = check_tiled_ensemble_size(B, members, g)) return rc;
    if (int rc = check_std_members(std_out, members)) return rc;
    if (!tiles || !mean_out) return fail(MI_EINVAL, "null argument");
    return launched(tile_blend_reduce_launch(tiles, B, members, g, mean_out, std_out, samples_out, (hipStream_t)stream), "tile_blend_reduce");
}

extern "C" int mi_tile_blend_quantiles(const float* tiles, int B, int members, int C, int H, int W, int th, int tw, int oy, int ox,
                                       const double* q, int nq, float* out, void* stream) {
    TileGeom g{};
    if (C < 1) return fail(MI_EINVAL, "C %d must be positive", C);
    if (int rc = fill_tile_geom(C, H, W, th, tw, oy, ox, &g)) return rc;
    if (int rc = check_tile_count(B, g)) return rc;
    if (int rc = check_step_noise_range(C, H, W, 0)) return rc;
    if (int rc = check_members_min(members)) return rc;
    if (int rc = check_reduce_batch(B, "the limit of mi_ensemble_quantiles, whose arithmetic this call composes")) return rc;      // (B >= 1: check_tile_count)
    if (int rc = check_tiled_ensemble_size(B, members, g)) return rc;
    if (int rc = check_quantile_members(members)) return rc;
    QuantileLevels ql;
    if (int rc = check_quantile_levels(q, nq, &ql)) return rc;
    if (!tiles || !out) return fail(MI_EINVAL, "null argument");
    return launched(tile_blend_quantiles_launch(tiles, B, members, g, ql, out, (hipStream_t)stream), "tile_blend_quantiles");
}

// Members are the outer loop: member m is mi_denoise_tiled's seeded pass structure with counter word c3 = member_offset + m, a
// launch constant of the update kernel, so no pass spans two members.  Its tiles are slice m of the storage [members][B][tiles].
extern "C" int mi_denoise_tiled_ensemble(mi_plan* plan, const float* noisy, float* mean_out, float* std_out, float* samples_out, float* tiles_out,
                                         int B, int members, int H, int W, int th, int tw, int oy, int ox,
                                         const int32_t* t_list, int n_iters,
                                         const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                         uint64_t seed, int64_t sample_offset, int64_t member_offset, int pass_samples, int flags,
                                         void* workspace, size_t workspace_bytes, void* stream) {
    TileGeom tg{};
    if (int rc = check_tiled_ensemble_args(plan, B, members, H, W, th, tw, oy, ox, sample_offset, member_offset, pass_samples, &tg)) return rc;
    if (!mean_out && !std_out && !samples_out && !tiles_out)
        return fail(MI_EINVAL, "no output: give at least one of mean_out, std_out, samples_out, tiles_out");
    if (int rc = check_std_members(std_out, members)) return rc;
    const int K = tg.ny * tg.nx;
    const size_t chw = (size_t)tg.C * th * tw, img = (size_t)tg.C * H * W * sizeof(float);
    const Buf buf[5] = {{noisy, (size_t)B * img, "noisy"}, {mean_out, (size_t)B * img, "mean_out"}, {std_out, (size_t)B * img, "std_out"},
                        {samples_out, (size_t)B * members * img, "samples_out"},
                        {tiles_out, (size_t)members * B * K * chw * sizeof(float), "tiles_out"}};
    if (int rc = check_no_overlap(buf, 5, "noisy is read by every pass and the reduce reads the tiles while it writes mean_out, std_out and samples_out"))
        return rc;
    const Schedule sc{t_list, n_iters, beta, alpha, alpha_hat, noise_steps};
    EnsembleLayout L{};
    // (evaluated before the state check, reported after it: check_batched_call; host arithmetic only, as in the *_workspace_bytes queries)
    const int layout_rc = tiled_ensemble_layout(plan, B, members, K, th, tw, pass_samples, tiles_out != nullptr, &L);
    if (int rc = check_batched_call(plan, layout_rc, L, workspace, workspace_bytes, {noisy}, sc)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* tiles = tiles_out ? tiles_out : reinterpret_cast<float*>(ws + L.samples_off);
    std::lock_guard<std::mutex> side_lk(plan->side_mu);     // held over all passes: the side streams are per plan
    HIPCHK(hipMemsetAsync(ws, 0, 256, s));                  // status word: once per call, the passes of every member accumulate into it
    StepNoise sn;
    sn.seeded = true; sn.seed = seed; sn.sample_offset = sample_offset; sn.members = K; sn.member_offset = (uint32_t)member_offset;
    sn.tiles_x = tg.nx; sn.tiles_y = tg.ny; sn.img_H = H; sn.img_W = W;
    auto extract = [&](float* cond, int v0, int n) { return launched(tile_extract_launch(noisy, cond, tg, v0, n, s), "tile_extract"); };
    if (int rc = run_passes(plan, extract, tiles, (int64_t)B * K, members, th, tw, chw, L, sn, sc, flags, ws, stream)) return rc;      // V: ONE member's
    if (mean_out || std_out || samples_out)
        return launched(tile_blend_reduce_launch(tiles, B, members, tg, mean_out, std_out, samples_out, s), "tile_blend_reduce");
    return MI_OK;
}

// ---------------------------------------------------------------------------- geometric self-ensemble: flip / rotate views
// the view list of a call, host int32 -> the kernel argument (include/midd.h: THE GEOMETRY)
static int check_views(const int32_t* views, int n_views, int H, int W, DihedralViews* dv) {
    if (n_views < 1 || n_views > DIHEDRAL_MAX_VIEWS)
        return fail(MI_EINVAL, "n_views %d outside [1, %d]: a view list holds 1 to 8 distinct view codes (limit: 1 <= n_views <= %d)", n_views,
                    DIHEDRAL_MAX_VIEWS, DIHEDRAL_MAX_VIEWS);
    if (!views) return fail(MI_EINVAL, "null argument: views");
    *dv = DihedralViews{};
    dv->n = n_views;
    for (int k = 0; k < n_views; ++k) {
        if (views[k] < 0 || views[k] > 7)
            return fail(MI_EINVAL, "views[%d] = %d outside [0, 7]: a view code is 4 * transpose + 2 * flip_rows + flip_columns (limit: 0 <= code <= 7)", k, views[k]);
        for (int j = 0; j < k; ++j)
            if (views[j] == views[k]) return fail(MI_EINVAL, "views[%d] = %d repeats views[%d]: the view codes of a list are distinct", k, views[k], j);
        dv->code[k] = (uint8_t)views[k];
    }
    for (int k = 0; k < n_views; ++k)
        if ((views[k] & 4) && H != W)
            return fail(MI_EINVAL, "views[%d] = %d transposes a %dx%d image: a pass never mixes image sizes (limit: view codes 4 .. 7 need H == W)", k, views[k], H, W);
    return MI_OK;
}

static int check_std_views(const float* std_out, int n_views) {
    if (std_out && n_views < 2) return fail(MI_EINVAL, "std_out needs at least two views: the unbiased standard deviation of one value is undefined");
    return MI_OK;
}

// what the three stand-alone calls share: the image shape, the view list, the batch
static int check_dihedral_call(int B, int C, int H, int W, const int32_t* views, int n_views, DihedralViews* dv) {
    if (C < 1) return fail(MI_EINVAL, "C %d must be positive", C);
    if (int rc = check_step_noise_range(C, H, W, 0)) return rc;
    if (int rc = check_views(views, n_views, H, W, dv)) return rc;
    return check_ensemble_size(B, n_views);
}

extern "C" int mi_dihedral_views(const float* images, int B, int C, int H, int W, const int32_t* views, int n_views,
                                 int v0, int n, float* dst, void* stream) {
    DihedralViews dv;
    if (int rc = check_dihedral_call(B, C, H, W, views, n_views, &dv)) return rc;
    if (v0 < 0 || n < 0 || n > 65535 || (int64_t)v0 + n > (int64_t)B * n_views)
        return fail(MI_EINVAL, "views [%d, %d + %d) outside the %d * %d virtual samples of the batch (limit per call: n <= 65535)", v0, v0, n, B, n_views);
    if (n == 0) return MI_OK;
    if (!images || !dst) return fail(MI_EINVAL, "null argument");
    return launched(dihedral_views_launch(images, dst, dv, C, H, W, v0, n, (hipStream_t)stream), "dihedral_views");
}

extern "C" int mi_dihedral_reduce(const float* views_out, int B, int C, int H, int W, const int32_t* views, int n_views,
                                  float* mean_out, float* std_out, float* samples_out, void* stream) {
    DihedralViews dv;
    if (int rc = check_dihedral_call(B, C, H, W, views, n_views, &dv)) return rc;
    if (!mean_out && !std_out && !samples_out) return fail(MI_EINVAL, "no output: give at least one of mean_out, std_out, samples_out");
    if (int rc = check_std_views(std_out, n_views)) return rc;
    if (!views_out) return fail(MI_EINVAL, "null argument");
    return launched(dihedral_reduce_launch(views_out, B, dv, C, H, W, mean_out, std_out, samples_out, (hipStream_t)stream), "dihedral_reduce");
}

extern "C" int mi_dihedral_quantiles(const float* views_out, int B, int C, int H, int W, const int32_t* views, int n_views,
                                     const double* q, int nq, float* out, void* stream) {
    DihedralViews dv;
    if (int rc = check_dihedral_call(B, C, H, W, views, n_views, &dv)) return rc;
    QuantileLevels ql;
    if (int rc = check_quantile_levels(q, nq, &ql)) return rc;
    if (!views_out || !out) return fail(MI_EINVAL, "null argument");
    return launched(dihedral_quantiles_launch(views_out, B, dv, C, H, W, ql, out, (hipStream_t)stream), "dihedral_quantiles");
}

// mi_denoise_ensemble with the views of an image in the place of its draws: virtual sample v = b * G + k is view k of image b.
// The sampler leaves every view's output in the view's own frame, always in the workspace (a transposing unview cannot run in
// place), and the reduce launch turns them back while it reads them.
extern "C" int mi_denoise_self_ensemble(mi_plan* plan, const float* noisy, float* mean_out, float* std_out, float* samples_out,
                                        int B, int H, int W, const int32_t* views, int n_views,
                                        const int32_t* t_list, int n_iters,
                                        const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                        int seeded, uint64_t seed, int64_t sample_offset, int64_t member_offset, int pass_samples, int flags,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    DihedralViews dv;
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (int rc = check_views(views, n_views, H, W, &dv)) return rc;      // the view list first, then the rules of an ensemble with one member per view
    if (int rc = check_ensemble_args(plan, B, n_views, H, W, sample_offset, member_offset, pass_samples)) return rc;
    if (!mean_out && !std_out && !samples_out) return fail(MI_EINVAL, "no output: give at least one of mean_out, std_out, samples_out");
    if (int rc = check_std_views(std_out, n_views)) return rc;
    const int Cc = plan->cfg.in_channels;
    const size_t chw = (size_t)Cc * H * W, img = chw * sizeof(float);
    const Buf buf[4] = {{noisy, (size_t)B * img, "noisy"}, {mean_out, (size_t)B * img, "mean_out"}, {std_out, (size_t)B * img, "std_out"},
                        {samples_out, (size_t)B * n_views * img, "samples_out"}};
    if (int rc = check_no_overlap(buf, 4, "noisy is read by every pass and the reduce writes mean_out, std_out and samples_out in one launch"))
        return rc;
    const Schedule sc{t_list, n_iters, beta, alpha, alpha_hat, noise_steps};
    EnsembleLayout L{};
    // (evaluated before the state check, reported after it: check_batched_call; host arithmetic only, as in the *_workspace_bytes queries)
    const int layout_rc = ensemble_layout(plan, B, n_views, H, W, pass_samples, false, &L);
    if (int rc = check_batched_call(plan, layout_rc, L, workspace, workspace_bytes, {noisy}, sc)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* views_out = reinterpret_cast<float*>(ws + L.samples_off);
    std::lock_guard<std::mutex> side_lk(plan->side_mu);     // held over all passes: the side streams are per plan
    HIPCHK(hipMemsetAsync(ws, 0, 256, s));                  // status word: once per call, the passes accumulate into it
    StepNoise sn;                                           // view k draws as member member_offset + k, at the pixel's place in the VIEW's frame
    if (seeded) { sn.seeded = true; sn.seed = seed; sn.sample_offset = sample_offset; sn.members = n_views; sn.member_offset = (uint32_t)member_offset; }
    auto fill = [&](float* cond, int v0, int n) { return launched(dihedral_views_launch(noisy, cond, dv, Cc, H, W, v0, n, s), "dihedral_views"); };
    if (int rc = run_passes(plan, fill, views_out, (int64_t)B * n_views, 1, H, W, chw, L, sn, sc, flags, ws, stream)) return rc;
    return launched(dihedral_reduce_launch(views_out, B, dv, Cc, H, W, mean_out, std_out, samples_out, s), "dihedral_reduce");
}

extern "C" int mi_debug_fetch(mi_plan* plan, const char* module_name, int B, int H, int W, const void* workspace,
                              float* dst, int* C, int* h, int* w, void* stream) {
    if (!plan || !module_name) return fail(MI_EINVAL, "null argument");
    Program* g = nullptr;
    int rc = get_program(plan, B, H, W, &g);
    if (rc) return rc;
    auto it = g->outputs.find(module_name);
    if (it == g->outputs.end()) return fail(MI_EINVAL, "module \"%s\" has no materialised output in this plan", module_name);
    const TensorRef& t = it->second;
    if (C) *C = t.C; if (h) *h = t.H; if (w) *w = t.W;
    if (dst) {
        if (!workspace) return fail(MI_EINVAL, "null workspace");
        return launched(nhwc_to_nchw_launch(reinterpret_cast<const float*>((const char*)workspace + t.off), dst, B, t.H, t.W, t.C,
                                            fp16_mfma(plan->cfg) ? 1 : 0, (hipStream_t)stream), "nhwc_to_nchw");
    }
    return MI_OK;
}

extern "C" int mi_profile_begin(mi_plan* plan) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    for (auto& sp : plan->spans) { plan->event_pool.push_back(sp.a); plan->event_pool.push_back(sp.b); }
    plan->spans.clear();
    plan->profiling = true;
    return MI_OK;
}

extern "C" int mi_profile_end(mi_plan* plan, mi_profile_entry* out, int max_entries, int* n_entries) {
    if (!plan || !n_entries) return fail(MI_EINVAL, "null argument");
    plan->profiling = false;
    std::map<std::string, mi_profile_entry> agg;
    std::vector<std::string> order;
    for (auto& sp : plan->spans) {
        HIPCHK(hipEventSynchronize(sp.b));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, sp.a, sp.b));
        auto it = agg.find(sp.name);
        if (it == agg.end()) {
            mi_profile_entry e{};
            snprintf(e.name, sizeof(e.name), "%s", sp.name.c_str());
            it = agg.emplace(sp.name, e).first;
            order.push_back(sp.name);
        }
        it->second.launches += 1; it->second.total_ms += ms; it->second.flops += sp.flops; it->second.bytes += sp.bytes;
        plan->event_pool.push_back(sp.a); plan->event_pool.push_back(sp.b);
    }
    plan->spans.clear();
    *n_entries = (int)order.size();
    for (int i = 0; i < (int)order.size() && i < max_entries && out; ++i) out[i] = agg[order[i]];
    if ((int)order.size() > max_entries) *n_entries = max_entries;
    return MI_OK;
}
