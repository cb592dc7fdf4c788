// Executor: walks a Program's launch list (run_program, mi_unet_forward), debug fetch and per-op profiling.
#include "midd_sampler.h"

using namespace midd;

int midd::run_program(mi_plan* p, Program* g, const StepIO& io, char* ws, int* status, hipStream_t s, hipEvent_t mid_event, int mid_div) {
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
        const char* out_symbol = nullptr;      // OP_OUT: the symbol its launch ran
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
                a.clamp_eps = io.clamp_eps;
                const StepNoise& n = io.sn;
                a.seeded = n.seeded; a.iter = io.iter; a.seed = n.seed; a.sample_offset = n.sample_offset;
                a.v0 = n.v0; a.members = n.members > 0 ? n.members : 1; a.member_offset = n.member_offset;
                a.tiles_x = n.tiles_x; a.tiles_y = n.tiles_y; a.img_H = n.img_H; a.img_W = n.img_W;
                e = out_conv_launch(a, io.update, s);
                out_symbol = out_conv_symbol(io.update, a.seeded);
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
            const size_t oc_at = out_symbol ? sp.name.find("out_conv_kernel") : std::string::npos;      // (op_work names the plain one)
            if (oc_at != std::string::npos) sp.name.replace(oc_at, 15, out_symbol);
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

int midd::check_device(mi_plan* plan) {
    int dev = -1;
    if (hipGetDevice(&dev) != hipSuccess || dev != plan->device)
        return fail(MI_ESTATE, "plan was finalized on device %d but current device is %d", plan->device, dev);
    return MI_OK;
}

int midd::check_finalized(mi_plan* plan) {
    return plan->finalized ? MI_OK : fail(MI_ESTATE, "mi_unet_finalize has not been called (or weights changed since)");
}

int midd::check_workspace(const void* ws, size_t got, size_t need) {
    if (!ws || got < need) return fail(MI_ENOMEM, "workspace too small: need %zu bytes, got %zu", need, got);
    if (((uintptr_t)ws) & 255) return fail(MI_EINVAL, "workspace must be 256-byte aligned");
    return MI_OK;
}

int midd::check_call(mi_plan* plan, int B, int H, int W, void* ws, size_t ws_bytes, Program** g) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (int rc = get_program(plan, B, H, W, g)) return rc;
    if (int rc = check_workspace(ws, ws_bytes, (*g)->bytes)) return rc;
    return check_device(plan);
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
