// The sampler loop and its rules: the uniform calls (mi_denoise and its siblings, one timestep per row) and the per-slot call
// (mi_denoise_slots), their schedules and coefficient tables, and the seeded step noise as a tensor.
#include "midd_sampler.h"

using namespace midd;

// every entry of a timestep list indexes the schedule's tables (check_schedule, check_ddim)
static int check_t_list(const int32_t* t, int n, int noise_steps) {
    for (int i = 0; i < n; ++i)
        if (t[i] < 0 || t[i] >= noise_steps) return fail(MI_EINVAL, "t_list[%d]=%d outside [0,%d)", i, t[i], noise_steps);
    return MI_OK;
}

// the sampler's host-side arguments (mi_denoise*, and the batched calls before their first pass)
int midd::check_schedule(mi_plan* plan, const Schedule& sc) {
    if ((sc.n > 0 && !sc.t) || !sc.beta || !sc.alpha || !sc.alpha_hat) return fail(MI_EINVAL, "null argument");
    if (sc.n < 0 || sc.noise_steps < 1 || sc.noise_steps > plan->time_rows)
        return fail(MI_EINVAL, "noise_steps %d exceeds the precomputed time table (%d rows)", sc.noise_steps, plan->time_rows);
    return check_t_list(sc.t, sc.n, sc.noise_steps);
}

// THE DDIM UPDATE, host side (include/midd.h): row i of the coefficient table of a list, in double precision from the caller's
// fp32 table, every value rounded once to fp32.  A = alpha_hat[t_i], P = alpha_hat[t_{i+1}], 1 after the last entry.  The one
// place that computes it: mi_ddim_coefficients exports it, enqueue_run passes its rows to the update kernel.
// A row is a function of the timestep and its neighbours in the list, -1 = none: the list forms below and the per-slot call
// (mi_denoise_slots_rule, mi_update_row), whose slots carry their neighbours across call boundaries, ask the same function.
static void ddim_row3(int t, int t_after, const float* alpha_hat, double eta, float out[7]) {
#pragma clang fp contract(off)
    const double A = (double)alpha_hat[t], P = t_after >= 0 ? (double)alpha_hat[t_after] : 1.0;
    const double sigma = eta * std::sqrt((1.0 - P) / (1.0 - A)) * std::sqrt(1.0 - A / P);
    const double rest = (1.0 - P) - sigma * sigma;
    out[0] = (float)(1.0 / std::sqrt(A)); out[1] = (float)std::sqrt(1.0 - A); out[2] = (float)std::sqrt(A); out[3] = (float)(1.0 / std::sqrt(1.0 - A));
    out[4] = (float)std::sqrt(P); out[5] = (float)std::sqrt(rest > 0.0 ? rest : 0.0); out[6] = (float)(2.0 * sigma);
}
static void ddim_row(const int32_t* t, int n, const float* alpha_hat, double eta, int i, float out[7]) {
    ddim_row3(t[i], i + 1 < n ? t[i + 1] : -1, alpha_hat, eta, out);
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
static float dpm_g3(int t_before, int t, int t_after, const float* alpha_hat) {
#pragma clang fp contract(off)
    if (t_before < 0 || t_after < 0) return 0.0f;
    const double Q = (double)alpha_hat[t_before], A = (double)alpha_hat[t], P = (double)alpha_hat[t_after];
    const double lA = dpm_lambda(A);
    const double h = dpm_lambda(P) - lA, h_prev = lA - dpm_lambda(Q);
    const double r = h_prev / h;
    const double emh = std::sqrt(((1.0 - P) / (1.0 - A)) * (A / P));      // e^{-h} without exp
    // the extrapolation weight 1 / (2 r) bounded at its uniform-step value 1/2 (why)
    return (float)(std::sqrt(P) * (1.0 - emh) / (2.0 * (r > 1.0 ? r : 1.0)));
}
static float dpm_g(const int32_t* t, int n, const float* alpha_hat, int i) {
    return dpm_g3(i > 0 ? t[i - 1] : -1, t[i], i + 1 < n ? t[i + 1] : -1, alpha_hat);
}

// the pair rule of check_ddim for one step of a list, t -> t_after (-1: the list ends, P = 1)
static int check_ddim_pair(int t, int t_after, const float* alpha_hat) {
    const double A = (double)alpha_hat[t], P = t_after >= 0 ? (double)alpha_hat[t_after] : 1.0;
    if (!(A > 0.0 && A < P && P <= 1.0))
        return fail(MI_EINVAL, "alpha_hat[%d]=%.9g, next %.9g: the DDIM update needs 0 < alpha_hat[t_i] < alpha_hat[t_{i+1}] <= 1", t, A, P);
    return MI_OK;
}

// One row of either table from the timestep and its neighbours (include/midd.h): the per-slot call's rows, for a caller to hold
extern "C" int mi_update_row(int32_t t_before, int32_t t, int32_t t_after, const float* alpha_hat, int noise_steps, double eta, float out[8]) {
    if (!(eta >= 0.0 && eta <= 1.0)) return fail(MI_EINVAL, "eta %.17g outside [0, 1] (limit: 0 <= eta <= 1, not NaN)", eta);
    if (!alpha_hat || !out) return fail(MI_EINVAL, "null argument");
    if (noise_steps < 1) return fail(MI_EINVAL, "noise_steps %d: a schedule has at least one step (limit: noise_steps >= 1)", noise_steps);
    if (t < 0 || t >= noise_steps) return fail(MI_EINVAL, "t=%d outside [0,%d)", t, noise_steps);
    if (t_before < -1 || t_before >= noise_steps || t_after < -1 || t_after >= noise_steps)
        return fail(MI_EINVAL, "t_before=%d / t_after=%d outside [-1,%d) (-1 = none)", t_before, t_after, noise_steps);
    if ((t_before >= 0 && t_before <= t) || t_after >= t)
        return fail(MI_EINVAL, "(t_before, t, t_after) = (%d, %d, %d): the DDIM update jumps from each timestep to the next one of the list "
                    "(limit: strictly decreasing, -1 = none)", t_before, t, t_after);
    if (t_before >= 0)
        if (int rc = check_ddim_pair(t_before, t, alpha_hat)) return rc;
    if (int rc = check_ddim_pair(t, t_after, alpha_hat)) return rc;
    ddim_row3(t, t_after, alpha_hat, eta, out);
    out[7] = dpm_g3(t_before, t, t_after, alpha_hat);
    return MI_OK;
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
int midd::apply_rule(const mi_update_rule* rule, Schedule* sc) {
    if (!rule || rule->kind == MI_UPDATE_REFERENCE) return MI_OK;
    if (rule->kind == MI_UPDATE_DPMPP2M)
        return fail(MI_EINVAL, "update rule MI_UPDATE_DPMPP2M needs a buffer for the predicted images, which this call does not take: "
                    "call mi_denoise_dpm or mi_denoise_tiled_dpm");
    if (rule->kind != MI_UPDATE_DDIM) return fail(MI_EINVAL, "unknown update rule %d (MI_UPDATE_REFERENCE or MI_UPDATE_DDIM)", (int)rule->kind);
    if (int rc = check_ddim(sc->t, sc->n, sc->alpha_hat, sc->noise_steps, rule->eta)) return rc;
    sc->rule = MI_UPDATE_DDIM; sc->eta = rule->eta; sc->clip_x0 = rule->clip_x0 ? 1 : 0;
    return MI_OK;
}

// mi_denoise_dpm and mi_denoise_tiled_dpm -> their Schedule: the rule's own cases (those of DDIM at eta 0) first, as apply_rule;
// x0 is the history in place (x0_stride 0; mi_denoise_dpm widens it to a trajectory)
int midd::apply_dpm(int clip_x0, float* x0, Schedule* sc) {
    if (int rc = check_ddim(sc->t, sc->n, sc->alpha_hat, sc->noise_steps, 0.0)) return rc;
    sc->rule = MI_UPDATE_DPMPP2M; sc->clip_x0 = clip_x0 ? 1 : 0; sc->x0 = x0;
    return MI_OK;
}

int midd::check_no_overlap(const Buf* b, int n, const char* why) {
    for (int i = 0; i < n; ++i)
        for (int j = i + 1; j < n; ++j) {
            const uintptr_t a = (uintptr_t)b[i].p, c = (uintptr_t)b[j].p;
            if (a && c && a < c + b[j].bytes && c < a + b[i].bytes)
                return fail(MI_EINVAL, "%s and %s alias (overlap): %s", b[i].name, b[j].name, why);
        }
    return MI_OK;
}

// One batch through the sampler loop, in two steps: check_run judges the arguments (no GPU work), enqueue_run enqueues the
// batch.  enqueue_run neither takes the plan's side-stream mutex nor clears the status word: its caller does both, once per
// C call -- denoise_run for the uniform calls, a batched call (midd_batched.hip) once for all its passes (run_passes), so that
// the word accumulates over them.
int midd::check_run(mi_plan* plan, const float* noisy, const float* x_out, int B, int H, int W, const Schedule& sc,
                    void* workspace, size_t workspace_bytes, Program** g) {
    int rc = check_call(plan, B, H, W, workspace, workspace_bytes, g);
    if (rc) return rc;
    if (!noisy || !x_out) return fail(MI_EINVAL, "null argument");
    if ((rc = check_schedule(plan, sc))) return rc;
    if (noisy == x_out) return fail(MI_EINVAL, "x_out must not alias noisy (the condition image is read every step)");
    return MI_OK;
}

// the reference's update of a sample at timestep t: fp32 arithmetic in the reference's order (DDIMModel.py:280-283)
static void reference_coeffs(const Schedule& sc, int t, float* c1, float* c2, float* c3) {
    *c1 = 1.0f / sqrtf(sc.alpha[t]);
    *c2 = (1.0f - sc.alpha[t]) / sqrtf(1.0f - sc.alpha_hat[t]);
    *c3 = sqrtf(sc.beta[t]);
}

// The update of row i of a uniform schedule for the samples from element `at` of the batch (a sub-batch's first), and whether
// the row has a noise term at all
static OutUpdate uniform_update(const Schedule& sc, int i, size_t at, bool* draws) {
    OutUpdate u{};
    *draws = sc.t[i] > 0;                                // nothing is drawn at t == 0
    if (sc.rule == MI_UPDATE_REFERENCE) {
        u.kind = OUT_REFERENCE;
        reference_coeffs(sc, sc.t[i], &u.ref.c1, &u.ref.c2, &u.ref.c3);
        return u;
    }
    float r[7];
    ddim_row(sc.t, sc.n, sc.alpha_hat, sc.eta, i, r);    // (eta is 0 under the multistep rule)
    const int last = i == sc.n - 1 ? 1 : 0;
    if (sc.rule == MI_UPDATE_DDIM) {
        u.kind = OUT_DDIM;
        u.ddim = DdimCoef{r[0], r[1], r[2], r[3], r[4], r[5], r[6], sc.clip_x0, last};
        *draws = r[6] > 0.0f;                            // nor at s == 0: every row at eta == 0, always the last one
    } else {
        u.kind = OUT_DPM;
        u.dpm.k = DpmCoef{r[0], r[1], r[2], r[3], r[4], r[5], dpm_g(sc.t, sc.n, sc.alpha_hat, i), sc.clip_x0, last};
        // iteration i reads slot i - 1 and writes slot i (in place when there is one slot)
        u.dpm.x0_out = sc.x0 + (size_t)i * sc.x0_stride + at;
        u.dpm.x0_prev = i > 0 ? sc.x0 + (size_t)(i - 1) * sc.x0_stride + at : u.dpm.x0_out;      // (i == 0: g == 0, not read)
        *draws = false;                                  // deterministic: no noise term
    }
    return u;
}

// Row i of mi_denoise_slots for the Bh columns from col0 of every table: their records leave as kernel arguments, SLOTS_PER_LAUNCH
// a launch, for recs[Bh], and their time-table rows for trow[Bh]
static int fill_slot_row(const Schedule& sc, const SlotRows& slots, bool has_noise, int i, int B, int H, int W, int col0, int Bh,
                         int* trow, SlotRec* recs, hipStream_t sh) {
    for (int c0 = 0; c0 < Bh; c0 += SLOTS_PER_LAUNCH) {
        SlotRecs r{};
        const int m = Bh - c0 < SLOTS_PER_LAUNCH ? Bh - c0 : SLOTS_PER_LAUNCH;
        for (int j = 0; j < m; ++j) {
            const int col = col0 + c0 + j, t = sc.t[(size_t)i * B + col];
            if (t < 0) continue;                             // idle: active 0, time row 0
            SlotRec& q = r.v[j];
            reference_coeffs(sc, t, &q.c1, &q.c2, &q.c3);
            q.active = SLOT_ACTIVE | ((t > 0 && has_noise) ? SLOT_NOISE : 0);      // nothing is drawn at t == 0
            q.iter = (unsigned)((slots.iter_base ? slots.iter_base[col] : 0) + i);
            q.image = (unsigned)(uint64_t)(slots.sample_index ? slots.sample_index[col] : (int64_t)col);
            q.trow = t;
            q.member = (unsigned)(uint64_t)(slots.member ? slots.member[col] : 0);
            const uint32_t* f = slots.frame ? slots.frame + (size_t)col * 3 : nullptr;
            q.pitch = f ? f[0] : (unsigned)W; q.plane = f ? f[1] : (unsigned)H * (unsigned)W; q.origin = f ? f[2] : 0u;
        }
        if (int rc = launched(slot_fill_launch(trow + c0, recs + c0, r, m, sh), "slot records")) return rc;
    }
    return MI_OK;
}

// The same row under a rule (mi_denoise_slots_rule): every record is the row of mi_update_row for the slot's own (previous, own, next)
// timesteps -- the neighbours inside the call from the table, those across its first and last row from t_before / t_after -- so a
// list cut into calls anywhere gives the coefficients of the list run whole.  g is the multistep rule's; eta is the DDIM rule's
static int fill_slot_rule_row(const Schedule& sc, const SlotRows& slots, bool has_noise, int i, int B, int H, int W, int col0, int Bh,
                              int* trow, SlotRuleRec* recs, hipStream_t sh) {
    for (int c0 = 0; c0 < Bh; c0 += SLOTS_PER_LAUNCH) {
        SlotRuleRecs r{};
        const int m = Bh - c0 < SLOTS_PER_LAUNCH ? Bh - c0 : SLOTS_PER_LAUNCH;
        for (int j = 0; j < m; ++j) {
            const int col = col0 + c0 + j, t = sc.t[(size_t)i * B + col];
            if (t < 0) continue;                             // idle: active 0, time row 0
            const int tb = i > 0 ? sc.t[(size_t)(i - 1) * B + col] : (slots.t_before ? slots.t_before[col] : -1);
            const int ta = i + 1 < sc.n ? sc.t[(size_t)(i + 1) * B + col] : (slots.t_after ? slots.t_after[col] : -1);
            SlotRuleRec& q = r.v[j];
            float k[7];
            ddim_row3(t, ta, sc.alpha_hat, sc.eta, k);       // (eta is 0 under the multistep rule)
            q.k0 = k[0]; q.k1 = k[1]; q.r0 = k[2]; q.r1 = k[3]; q.a = k[4]; q.b = k[5]; q.s = k[6];
            q.g = sc.rule == MI_UPDATE_DPMPP2M ? dpm_g3(tb, t, ta, sc.alpha_hat) : 0.0f;
            q.active = SLOT_ACTIVE | ((q.s > 0.0f && has_noise) ? SLOT_NOISE : 0) | (ta < 0 ? SLOT_LAST : 0) | (q.g != 0.0f ? SLOT_HIST : 0);
            q.iter = (unsigned)((slots.iter_base ? slots.iter_base[col] : 0) + i);
            q.image = (unsigned)(uint64_t)(slots.sample_index ? slots.sample_index[col] : (int64_t)col);
            q.trow = t;
            q.member = (unsigned)(uint64_t)(slots.member ? slots.member[col] : 0);
            const uint32_t* f = slots.frame ? slots.frame + (size_t)col * 3 : nullptr;
            q.pitch = f ? f[0] : (unsigned)W; q.plane = f ? f[1] : (unsigned)H * (unsigned)W; q.origin = f ? f[2] : 0u;
        }
        if (int rc = launched(slot_rule_fill_launch(trow + c0, recs + c0, r, m, sh), "slot rule records")) return rc;
    }
    return MI_OK;
}

// (the caller holds plan->side_mu and has cleared the status word at the head of `workspace`)
int midd::enqueue_run(mi_plan* plan, Program* g, const float* noisy, float* x_out, int B, int H, int W,
                      const Schedule& sc, const SlotRows* slots, const StepNoise& sn, int flags,
                      void* workspace, size_t workspace_bytes, void* stream) {
    const int n_iters = sc.n;
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
                int* trow = reinterpret_cast<int*>(wsh + gh->trow_off);
                StepIO io{};
                io.x = x_out + h * part; io.cond = noisy + h * part; io.eps_out = nullptr; io.x_update = x_out + h * part;
                if (slots && sc.rule != MI_UPDATE_REFERENCE) {
                    // the same under a rule: the larger records in the same region, and the sub-batch's columns of the history
                    SlotRuleRec* recs = reinterpret_cast<SlotRuleRec*>(wsh + gh->slot_off);
                    if (int rc2 = fill_slot_rule_row(sc, *slots, sn.seeded || sn.tensor, i, B, H, W, h * Bh, Bh, trow, recs, sh)) return rc2;
                    io.update.kind = OUT_SLOTS_RULE;
                    io.update.slots_rule = SlotRuleStep{recs, sc.clip_x0, sc.x0 ? sc.x0 + h * part : nullptr};
                    io.noise = sn.tensor ? sn.tensor + (size_t)i * img_elems + h * part : nullptr;
                    io.sn.seeded = sn.seeded; io.sn.seed = sn.seed;
                } else if (slots) {
                    // sub-batch h takes columns [h * Bh, (h + 1) * Bh) of every table
                    SlotRec* recs = reinterpret_cast<SlotRec*>(wsh + gh->slot_off);
                    if (int rc2 = fill_slot_row(sc, *slots, sn.seeded || sn.tensor, i, B, H, W, h * Bh, Bh, trow, recs, sh)) return rc2;
                    io.update.kind = OUT_SLOTS; io.update.slots = recs;
                    io.noise = sn.tensor ? sn.tensor + (size_t)i * img_elems + h * part : nullptr;
                    io.sn.seeded = sn.seeded; io.sn.seed = sn.seed;
                } else {
                    HIPCHK(hipMemsetD32Async((hipDeviceptr_t)trow, sc.t[i], Bh, sh));          // t = full((B,), i)
                    bool draws;
                    io.update = uniform_update(sc, i, h * part, &draws);
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

// the generator's counter words: element index and sample index (step_noise_common.h)
int midd::check_step_noise_range(int64_t C, int64_t H, int64_t W, int64_t sample_offset) {
    if (sample_offset < 0) return fail(MI_EINVAL, "sample_offset %lld is negative: the global sample index starts at 0", (long long)sample_offset);
    if (C < 1 || H < 1 || W < 1) return fail(MI_EINVAL, "bad image shape %lldx%lldx%lld", (long long)C, (long long)H, (long long)W);
    // (three factors below 2^31 each: the product of two fits 64 bits, the third is compared by division)
    if (C * H > (int64_t)0xFFFFFFFFll / W)
        return fail(MI_EINVAL, "C*H*W = %lld*%lld*%lld reaches 2^32: the element index of the seeded step noise is one 32-bit counter word "
                    "(limit: C*H*W < 4294967296)", (long long)C, (long long)H, (long long)W);
    return MI_OK;
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
        if (!plan) return fail(MI_EINVAL, "null plan");      // (the counter range needs the plan; unseeded, check_call answers)
        if (int rc = check_step_noise_range(plan->cfg.in_channels, H, W, sample_offset)) return rc;
        sn.seeded = true; sn.seed = seed; sn.sample_offset = sample_offset;
    } else {
        sn.tensor = step_noise;
    }
    return denoise_run(plan, noisy, x_out, B, H, W, sc, sn, flags, workspace, workspace_bytes, stream);
}

extern "C" int mi_denoise(mi_plan* plan, const float* noisy, float* x_out, int B, int H, int W,
                          const int32_t* t_list, int n_iters,
                          const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                          const float* step_noise, int flags,
                          void* workspace, size_t workspace_bytes, void* stream) {
    return mi_denoise_rule(plan, noisy, x_out, B, H, W, t_list, n_iters, beta, alpha, alpha_hat, noise_steps, step_noise, 0, 0, 0, flags,
                           nullptr, workspace, workspace_bytes, stream);
}

extern "C" int mi_denoise_seeded(mi_plan* plan, const float* noisy, float* x_out, int B, int H, int W,
                                 const int32_t* t_list, int n_iters,
                                 const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                 uint64_t seed, int64_t sample_offset, int flags,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    return mi_denoise_rule(plan, noisy, x_out, B, H, W, t_list, n_iters, beta, alpha, alpha_hat, noise_steps, nullptr, 1, seed, sample_offset, flags,
                           nullptr, workspace, workspace_bytes, stream);
}

// The second-order multistep rule (include/midd.h: THE DPMPP2M UPDATE): mi_denoise plus the caller's buffer of predicted images
extern "C" int mi_denoise_dpm(mi_plan* plan, const float* noisy, float* x_out, float* x0_buf, int x0_slots, int B, int H, int W,
                              const int32_t* t_list, int n_iters,
                              const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                              int flags, int clip_x0, void* workspace, size_t workspace_bytes, void* stream) {
    Schedule sc{t_list, n_iters, beta, alpha, alpha_hat, noise_steps};
    if (int rc = apply_dpm(clip_x0, x0_buf, &sc)) return rc;      // the rule's own cases first, as mi_denoise_rule
    if (x0_slots != 1 && x0_slots != n_iters)
        return fail(MI_EINVAL, "x0_slots %d: 1 (the history in place) or n_iters = %d (the trajectory of predicted images)", x0_slots, n_iters);
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (n_iters > 0 && !x0_buf) return fail(MI_EINVAL, "null argument");
    if (B < 1 || H < 1 || W < 1) return fail(MI_EINVAL, "bad image shape %dx%dx%d", B, H, W);
    const size_t img_elems = (size_t)B * plan->cfg.in_channels * H * W;
    const Buf buf[3] = {{noisy, img_elems * sizeof(float), "noisy"}, {x_out, img_elems * sizeof(float), "x_out"},
                        {x0_buf, (size_t)x0_slots * img_elems * sizeof(float), "x0_buf"}};
    if (int rc = check_no_overlap(buf, 3, "noisy is read every step and x0_buf is written beside x_out")) return rc;
    sc.x0_stride = x0_slots > 1 ? img_elems : 0;
    return denoise_run(plan, noisy, x_out, B, H, W, sc, StepNoise{}, flags, workspace, workspace_bytes, stream);
}

// ---------------------------------------------------------------------------- per-slot timesteps (continuous batching)
// The rule's own column rules (mi_denoise_slots_rule), after the table's entries have been judged: per column, the sequence
// (t_before, the active rows, t_after) is a piece of a DDIM list -- strictly decreasing, every step within check_ddim's alpha_hat rule
static int check_rule_columns(const int32_t* t_rows, int n_rows, int B, const int32_t* t_before, const int32_t* t_after,
                              const float* alpha_hat, int noise_steps) {
    for (int b = 0; b < B; ++b) {
        const int tb = t_before ? t_before[b] : -1, ta = t_after ? t_after[b] : -1;
        if (tb < -1 || tb >= noise_steps) return fail(MI_EINVAL, "t_before[%d]=%d outside [-1,%d) (-1 = none)", b, tb, noise_steps);
        if (ta < -1 || ta >= noise_steps) return fail(MI_EINVAL, "t_after[%d]=%d outside [-1,%d) (-1 = none)", b, ta, noise_steps);
        int prev = tb, rows = 0;
        for (int i = 0; i < n_rows; ++i) {
            const int t = t_rows[(size_t)i * B + b];
            if (t < 0) break;                                // (active on a prefix of the rows: judged before)
            if (prev >= 0 && t >= prev)
                return fail(MI_EINVAL, "t_rows[%d][%d]=%d after %s=%d: the update jumps from each timestep of a slot to its next one "
                            "(limit: a strictly decreasing column, t_before and t_after included)", i, b, t, i ? "the row above" : "t_before", prev);
            if (prev >= 0)
                if (int rc = check_ddim_pair(prev, t, alpha_hat)) return rc;
            prev = t; ++rows;
        }
        if (ta >= 0 && rows < n_rows)
            return fail(MI_EINVAL, "t_after[%d]=%d: slot %d went idle inside the call, its list has ended (limit: t_after = -1 after an idle row)", b, ta, b);
        if (ta >= 0 && prev >= 0 && ta >= prev)
            return fail(MI_EINVAL, "t_after[%d]=%d after t_rows[%d][%d]=%d: the update jumps from each timestep of a slot to its next one "
                        "(limit: a strictly decreasing column, t_before and t_after included)", b, ta, n_rows - 1, b, prev);
        if (rows > 0)
            if (int rc = check_ddim_pair(prev, ta, alpha_hat)) return rc;
    }
    return MI_OK;
}

// The three slot calls in one body, so the same rules in the same order and the same launches.  rule == null: the reference's
// update (t_before, t_after and x0_hist are null); else a judged MI_UPDATE_DDIM / MI_UPDATE_DPMPP2M rule of mi_denoise_slots_rule
static int slots_run(mi_plan* plan, const float* cond, float* x, int B, int H, int W,
                     const int32_t* t_rows, int n_rows, const int32_t* iter_base, const int64_t* sample_index,
                     const int64_t* member, const uint32_t* frame, const int32_t* t_before, const int32_t* t_after, float* x0_hist,
                     const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                     const float* step_noise, int seeded, uint64_t seed, int flags, const mi_update_rule* rule,
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
    } else if (member || frame) {
        return fail(MI_EINVAL, "%s without seeded: the table holds counter words of the seeded generator, a step_noise tensor is already "
                    "per slot (limit: member and frame need seeded != 0)", member ? "member" : "frame");
    }
    for (int b = 0; member && b < B; ++b)
        if (member[b] < 0 || member[b] >= ((int64_t)1 << 32))
            return fail(MI_EINVAL, "member[%d]=%lld outside [0, 2^32): the member index is one 32-bit counter word (limit: member < 4294967296)",
                        b, (long long)member[b]);
    for (int b = 0; frame && b < B; ++b) {
        const uint64_t pitch = frame[(size_t)b * 3], plane = frame[(size_t)b * 3 + 1], origin = frame[(size_t)b * 3 + 2];
        if (pitch < (uint64_t)W)
            return fail(MI_EINVAL, "frame[%d]: pitch %llu is less than the slot's width %d (limit: pitch >= W)", b, (unsigned long long)pitch, W);
        if (origin + (uint64_t)(H - 1) * pitch + (uint64_t)W > plane)
            return fail(MI_EINVAL, "frame[%d]: origin %llu + (H-1)*pitch + W = %llu leaves the plane of %llu elements "
                        "(limit: origin + (H-1)*pitch + W <= plane)", b, (unsigned long long)origin,
                        (unsigned long long)(origin + (uint64_t)(H - 1) * pitch + (uint64_t)W), (unsigned long long)plane);
        if ((uint64_t)plan->cfg.in_channels * plane >= (1ull << 32))
            return fail(MI_EINVAL, "frame[%d]: C*plane = %d*%llu reaches 2^32: the element index of the seeded step noise is one 32-bit "
                        "counter word (limit: C*plane < 4294967296)", b, plan->cfg.in_channels, (unsigned long long)plane);
    }
    if (rule)
        if (int rc = check_rule_columns(t_rows, n_rows, B, t_before, t_after, alpha_hat, noise_steps)) return rc;
    const size_t batch_bytes = (size_t)B * plan->cfg.in_channels * H * W * sizeof(float);
    const Buf buf[3] = {{x, batch_bytes, "x"}, {cond, batch_bytes, "cond"}, {x0_hist, batch_bytes, "x0_hist"}};
    if (int rc = check_no_overlap(buf, 2, "the condition images are read by every row while x is updated in place")) return rc;
    if (int rc = check_no_overlap(buf, 3, "x0_hist is read and written beside x by every row")) return rc;
    if (int rc = check_finalized(plan)) return rc;
    if (noise_steps > plan->time_rows)
        return fail(MI_EINVAL, "noise_steps %d exceeds the precomputed time table (%d rows)", noise_steps, plan->time_rows);
    Program* g = nullptr;
    if (int rc = check_call(plan, B, H, W, workspace, workspace_bytes, &g)) return rc;
    if (n_rows == 0) return MI_OK;
    StepNoise sn;
    sn.tensor = step_noise; sn.seeded = seeded != 0; sn.seed = seed;
    const SlotRows slots{iter_base, sample_index, member, frame, t_before, t_after};
    Schedule sc{t_rows, n_rows, beta, alpha, alpha_hat, noise_steps};
    if (rule) { sc.rule = rule->kind; sc.eta = rule->kind == MI_UPDATE_DDIM ? rule->eta : 0.0; sc.clip_x0 = rule->clip_x0 ? 1 : 0; sc.x0 = x0_hist; }
    std::lock_guard<std::mutex> side_lk(plan->side_mu);
    HIPCHK(hipMemsetAsync(workspace, 0, 256, (hipStream_t)stream));      // status word: once per call
    return enqueue_run(plan, g, cond, x, B, H, W, sc, &slots, sn, flags, workspace, workspace_bytes, stream);
}

// mi_denoise_slots is this call with member == frame == NULL
extern "C" int mi_denoise_slots_virtual(mi_plan* plan, const float* cond, float* x, int B, int H, int W,
                                        const int32_t* t_rows, int n_rows, const int32_t* iter_base, const int64_t* sample_index,
                                        const int64_t* member, const uint32_t* frame,
                                        const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                        const float* step_noise, int seeded, uint64_t seed, int flags,
                                        void* workspace, size_t workspace_bytes, void* stream) {
    return slots_run(plan, cond, x, B, H, W, t_rows, n_rows, iter_base, sample_index, member, frame, nullptr, nullptr, nullptr,
                     beta, alpha, alpha_hat, noise_steps, step_noise, seeded, seed, flags, nullptr, workspace, workspace_bytes, stream);
}

// The per-slot call under an update rule (include/midd.h).  What the rule itself refuses is judged first, before the table, the
// plan's state and any GPU work, as in the other *_rule calls
extern "C" int mi_denoise_slots_rule(mi_plan* plan, const float* cond, float* x, int B, int H, int W,
                                     const int32_t* t_rows, int n_rows, const int32_t* iter_base, const int64_t* sample_index,
                                     const int64_t* member, const uint32_t* frame,
                                     const int32_t* t_before, const int32_t* t_after, float* x0_hist,
                                     const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                     const float* step_noise, int seeded, uint64_t seed, int flags,
                                     const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream) {
    if (!rule || rule->kind == MI_UPDATE_REFERENCE) {
        if (t_before || t_after || x0_hist)
            return fail(MI_EINVAL, "%s with the reference's update: t_before, t_after and x0_hist belong to MI_UPDATE_DDIM / MI_UPDATE_DPMPP2M "
                        "(limit: all three NULL under MI_UPDATE_REFERENCE)", t_before ? "t_before" : t_after ? "t_after" : "x0_hist");
        return slots_run(plan, cond, x, B, H, W, t_rows, n_rows, iter_base, sample_index, member, frame, nullptr, nullptr, nullptr,
                         beta, alpha, alpha_hat, noise_steps, step_noise, seeded, seed, flags, nullptr, workspace, workspace_bytes, stream);
    }
    if (rule->kind == MI_UPDATE_DDIM) {
        if (!(rule->eta >= 0.0 && rule->eta <= 1.0)) return fail(MI_EINVAL, "eta %.17g outside [0, 1] (limit: 0 <= eta <= 1, not NaN)", rule->eta);
        if (x0_hist) return fail(MI_EINVAL, "x0_hist with MI_UPDATE_DDIM: the rule keeps no predicted image (limit: x0_hist NULL; MI_UPDATE_DPMPP2M takes it)");
    } else if (rule->kind == MI_UPDATE_DPMPP2M) {
        if (!x0_hist) return fail(MI_EINVAL, "MI_UPDATE_DPMPP2M without x0_hist: the rule reads every slot's previous predicted image (limit: x0_hist [B,C,H,W] on the device)");
        if (seeded || step_noise)
            return fail(MI_EINVAL, "%s with MI_UPDATE_DPMPP2M: the rule is deterministic, it has no noise term (limit: seeded == 0, step_noise NULL)",
                        seeded ? "seeded" : "step_noise");
    } else {
        return fail(MI_EINVAL, "unknown update rule %d (MI_UPDATE_REFERENCE, MI_UPDATE_DDIM or MI_UPDATE_DPMPP2M)", (int)rule->kind);
    }
    return slots_run(plan, cond, x, B, H, W, t_rows, n_rows, iter_base, sample_index, member, frame, t_before, t_after, x0_hist,
                     beta, alpha, alpha_hat, noise_steps, step_noise, seeded, seed, flags, rule, workspace, workspace_bytes, stream);
}

extern "C" int mi_denoise_slots(mi_plan* plan, const float* cond, float* x, int B, int H, int W,
                                const int32_t* t_rows, int n_rows, const int32_t* iter_base, const int64_t* sample_index,
                                const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                const float* step_noise, int seeded, uint64_t seed, int flags,
                                void* workspace, size_t workspace_bytes, void* stream) {
    return mi_denoise_slots_virtual(plan, cond, x, B, H, W, t_rows, n_rows, iter_base, sample_index, nullptr, nullptr, beta, alpha, alpha_hat,
                                    noise_steps, step_noise, seeded, seed, flags, workspace, workspace_bytes, stream);
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
