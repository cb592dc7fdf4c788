// Execution planner: (plan, B, H, W) -> Program (the launch list with its tiles, workspace offsets and statistics arena),
// the program cache, the workspace size, and the host-only plan dump.
#include "midd_host.h"

using namespace midd;

// One planned convolution.  The first six fields are given positionally, everything else by name.
struct ConvSpec {
    const TensorRef* s0; const TensorRef* s1;   // sources: s1 != null is the virtual torch.cat
    TensorRef* dst;                             // gets its statistics id when want_stats
    size_t w, b; float wscale;                  // packed weights, bias, output scale of the packing (Mod)
    bool wide = false; size_t w_wide = 0;       // wide: finalize packs a wide-chunk copy of these weights (at w_wide) when packs_wide_copy(Cin)
    int ks = 3, stride = 1, temb_col = -1;      // temb_col: column of the time table added to the output
    int prologue = PRO_RAW; GnRef gn{};         // GroupNorm (+ SiLU) of the sources applied while staging, with its affine
    const TensorRef* resid = nullptr;           // added in the epilogue
    bool want_stats = true;                     // leave the GroupNorm totals of the output
    float raw_scale_fixed = 1.0f;               // prologue RAW, sources without totals: fixed prescale of the operand
    int att_mode = ATT_NONE; size_t att_scratch = 0; int att_ksplit = 1;      // attention hand-off of the 1x1 kernel
    const TensorRef* res0 = nullptr; const TensorRef* res1 = nullptr; float res_wscale = 1.f;   // folded res_conv: the block input (virtual cat), scale of its packing
};

struct Builder {
    mi_plan* p; Program* g; int B;
    size_t cur = 0;             // workspace bump allocator, 256-byte aligned
    size_t take(size_t bytes) { size_t o = (cur + 255) & ~(size_t)255; cur = o + bytes; return o; }
    TensorRef alloc(int C, int H, int W) {
        TensorRef t; t.C = C; t.H = H; t.W = W;
        t.off = take((size_t)B * H * W * C * sizeof(float));
        return t;
    }
    // Totals live in one arena so ONE memset clears them all.  A tensor's totals are kept per block of `bs` channels: the
    // largest size every consuming GroupNorm's groups are whole multiples of (consumers register with gn_consumer).
    struct StatInfo { int C, bs; size_t off; };
    std::vector<StatInfo> stats;
    static int gcd(int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; }
    void alloc_stats(TensorRef& t) { t.stat_id = (int)stats.size(); stats.push_back(StatInfo{t.C, t.C, 0}); }
    // GroupNorm(8, C0 + C1) over (s0 [, s1]): group boundaries lie at multiples of cg from the start of s0
    int gn_consumer(const TensorRef& s0, const TensorRef* s1) {
        if (s0.stat_id < 0 || (s1 && s1->stat_id < 0)) return fail(MI_EINVAL, "internal: GroupNorm input without statistics");
        const int cg = (s0.C + (s1 ? s1->C : 0)) / GN_GROUPS_;
        stats[s0.stat_id].bs = gcd(stats[s0.stat_id].bs, cg);
        if (s1) stats[s1->stat_id].bs = gcd(gcd(stats[s1->stat_id].bs, cg), s0.C % cg);      // gcd(x, 0) == x
        return MI_OK;
    }
    // per-channel totals for a tensor no MFMA convolution produced
    void ensure_stats(TensorRef& t) {
        if (t.stat_id >= 0) return;
        alloc_stats(t);
        Op o{}; o.kind = OP_CHAN_TOT; o.s0 = t; o.stat_rows = chan_partial_rows(t.H * t.W, t.C); g->ops.push_back(o);
    }
    int conv(const ConvSpec& c) {
        const TensorRef &s0 = *c.s0, *s1 = c.s1; TensorRef& dst = *c.dst;
        const int cin = s0.C + (s1 ? s1->C : 0);
        const bool f16 = fp16_mfma(p->cfg);
        Op o{}; o.kind = OP_CONV; o.att_mode = c.att_mode; o.partial_off = c.att_scratch; o.att_ksplit = c.att_ksplit; o.s0 = s0; if (s1) { o.s1 = *s1; o.has_s1 = true; }
        // wscale = 2^-k / 2^s undoes the weight and the activation prescale; a raw operand's own prescale (per sample from
        // its statistics, or raw_scale_fixed) is divided out inside the kernel
        o.out_scale = (c.prologue == PRO_RAW && f16) ? c.wscale * ACT_PRESCALE_H : c.wscale;
        o.raw_scale_fixed = c.raw_scale_fixed;
        o.raw_stats = c.prologue == PRO_RAW && s0.stat_id >= 0 && (!s1 || s1->stat_id >= 0);
        o.w = c.w; o.b = c.b; o.ks = c.ks; o.stride = c.stride; o.prologue = c.prologue; o.temb_col = c.temb_col; o.gn = c.gn;
        if (c.gn.on) { if (int rcg = gn_consumer(s0, s1)) return rcg; }
        if (c.resid) { o.resid = *c.resid; o.has_resid = true; }
        if (c.res0) {
            o.res0 = *c.res0; if (c.res1) { o.res1 = *c.res1; o.has_res1 = true; }
            o.res_steps = (c.res0->C + (c.res1 ? c.res1->C : 0) + 31) / 32;
            o.res_scale = c.res_wscale * ACT_PRESCALE_H;         // 2^-k of the res_conv weights
        }
        const int Bp = p->batch_invariant ? INVARIANT_B : B; // batch-invariant plans tile as for the canonical batch
        const bool ok = f16 ? conv16_pick_tile(cin, dst.C, Bp, dst.H, dst.W, c.ks, c.stride, &o.tile, g->wide_chunks && c.wide && packs_wide_copy(p->cfg, cin), operand_planes(p->cfg))
                            : conv_pick_tile(dst.C, Bp, dst.H, dst.W, c.ks, c.stride, &o.tile);
        if (!ok) return fail(MI_EINVAL, "no conv tile for Cout=%d ks=%d stride=%d", dst.C, c.ks, c.stride);
        if (o.tile.cb == 2) o.w = c.w_wide;                  // the launch walks K in the wide order
        if (c.att_mode == ATT_PART_IN) o.tile.mt = 1;        // 64-pixel tiles: the partials of up to four splits x two K steps live in registers
        if (c.want_stats) { alloc_stats(dst); o.want_stats = true; }
        o.dst = dst;
        g->ops.push_back(o);
        return MI_OK;
    }
};

static int build_program(mi_plan* p, int B, int H, int W, Program* g) {
    const mi_unet_cfg& c = p->cfg;
    const int div = 1 << (p->levels - 1);
    if (B < 1 || H < div || W < div || H % div || W % div)
        return fail(MI_EINVAL, "H and W must be positive multiples of %d (got %dx%d), B >= 1", div, H, W);
    g->B = B; g->H = H; g->W = W;
    // ~640 persistent workgroups per launch, i.e. 640 / B per sample, each adding to the totals once: ~48 per copy
    g->stat_rep = (640 / B + 47) / 48;
    if (g->stat_rep < 1) g->stat_rep = 1;
    if (g->stat_rep > STAT_MAX_REPLICAS) g->stat_rep = STAT_MAX_REPLICAS;
    Builder bld{p, g, B};
    (void)bld.take(256);                      // [0, 256): the call's status word (mi_status); sub-batch programs leave theirs unused
    g->trow_off = bld.take((size_t)B * sizeof(int));
    g->slot_off = bld.take((size_t)B * sizeof(SlotRuleRec));  // mi_denoise_slots / mi_denoise_slots_rule: this row's record of every sample, sized for the larger of the two
    int rc;

    auto run_rb = [&](const Mod& m, const TensorRef& s0, const TensorRef* s1, TensorRef* out) -> int {
        const int cin = s0.C + (s1 ? s1->C : 0);
        if (cin != m.in_c) return fail(MI_EINVAL, "%s: expected %d input channels, graph provides %d", m.name.c_str(), m.in_c, cin);
        TensorRef h1 = bld.alloc(m.out_c, s0.H, s0.W);
        TensorRef o = bld.alloc(m.out_c, s0.H, s0.W), acc;
        ConvSpec c1{&s0, s1, &h1, m.w1, m.b1, m.s1};
        c1.wide = true; c1.w_wide = m.w1x; c1.prologue = PRO_GN_SILU; c1.gn = GnRef{m.g1, m.be1, true}; c1.temb_col = m.temb_col;
        if ((rc = bld.conv(c1))) return rc;
        ConvSpec c2{&h1, nullptr, &o, m.w2, m.b2, m.s2};
        c2.wide = true; c2.w_wide = m.w2x; c2.prologue = PRO_GN_SILU; c2.gn = GnRef{m.g2, m.be2, true};
        if (m.in_c != m.out_c && fp16_mfma(p->cfg)) {
            // res_conv(x) inside conv2's launch: extra K steps over the block input after each tile's 3x3 steps (SURVEY 2.1;
            // round 2 ran it as a launch of its own that wrote the tensor conv2 then re-read as its residual operand)
            c2.b = m.b2r; c2.res0 = &s0; c2.res1 = s1; c2.res_wscale = m.sr;
        } else if (m.in_c != m.out_c) {
            // fp32 MFMA mode: res_conv(x) as a launch of its own, added by conv2's epilogue
            ConvSpec cr{&s0, s1, &o, m.wr, m.br, m.sr};
            cr.ks = 1; cr.want_stats = false;
            if ((rc = bld.conv(cr))) return rc;
            acc = o; c2.resid = &acc;                              // + in place
        } else {
            if (s1) return fail(MI_EINVAL, "%s: identity residual over a concatenated input", m.name.c_str());
            c2.resid = &s0;
        }
        if ((rc = bld.conv(c2))) return rc;
        *out = o;
        return MI_OK;
    };
    auto run_attn = [&](const Mod& m, const TensorRef& x, TensorRef* out) -> int {
        const int C = x.C, N = x.H * x.W;
        const bool f16 = fp16_mfma(p->cfg);
        TensorRef y = bld.alloc(C, x.H, x.W);
        // fp32 MFMA mode: qkv tensor -> attention -> att tensor -> proj.
        // split-fp16 mode, three launches: the qkv projection's epilogue writes q (fp32 [B][N][C], the head of `qkv`'s buffer)
        // and the split-fp16 K / V images into the scratch; the attention kernel leaves key-split partials there; the
        // output projection combines them while it loads its operand
        const Att16Layout lay = attention16_layout(B, N, C, operand_planes(p->cfg));
        const size_t scratch = f16 ? bld.take(lay.bytes) : 0;
        int ksplit = 1, tps = 1;
        if (f16) attention16_split(N, ATTN_HEADS_ABI, p->batch_invariant ? INVARIANT_B : B, &ksplit, &tps);
        TensorRef qkv = bld.alloc(3 * C, x.H, x.W);            // Cout of the projection; f16x3: only [B][N][C] floats (q) are written
        ConvSpec cq{&x, nullptr, &qkv, m.wq, m.bq, m.sq};
        cq.ks = 1; cq.prologue = PRO_GN; cq.gn = GnRef{m.g1, m.be1, true}; cq.want_stats = false;
        if (f16) { cq.att_mode = ATT_QKV_OUT; cq.att_scratch = scratch; cq.att_ksplit = ksplit; }
        if ((rc = bld.conv(cq))) return rc;
        TensorRef att{}; att.off = scratch + lay.po_off; att.C = C; att.H = x.H; att.W = x.W;        // f16x3: split 0 of the partials [ksplit][B][N][C]
        if (!f16) att = bld.alloc(C, x.H, x.W);
        Op o{}; o.kind = OP_ATTN; o.s0 = qkv; o.dst = f16 ? y : att; o.partial_off = scratch; o.att_ksplit = ksplit; o.att_tps = tps;
        g->ops.push_back(o);
        ConvSpec cp{&att, nullptr, &y, m.wp, m.bp, m.sp};
        cp.ks = 1; cp.resid = &x;
        // f16x3: |att| <= max|v|, and 16 v is within fp16 (checked by the qkv epilogue): fixed prescale 2^4
        if (f16) { cp.raw_scale_fixed = ACT_PRESCALE_H; cp.att_mode = ATT_PART_IN; cp.att_scratch = scratch; cp.att_ksplit = ksplit; }
        if ((rc = bld.conv(cp))) return rc;
        *out = y;
        return MI_OK;
    };

    TensorRef h = bld.alloc(c.model_channels, H, W);
    { Op o{}; o.kind = OP_IN_CONV; bld.alloc_stats(h); o.dst = h; g->ops.push_back(o); }       // in_conv leaves its own totals
    g->outputs["in_conv"] = h;
    std::vector<TensorRef> skips;
    auto run_block = [&](const Mod& m) -> int {          // a residual or attention block on h
        TensorRef o;
        if ((rc = m.kind == MOD_RB ? run_rb(m, h, nullptr, &o) : run_attn(m, h, &o))) return rc;
        h = o; g->outputs[m.name] = h;
        return MI_OK;
    };
    for (const Mod& m : p->downs) {
        if (m.kind == MOD_DOWN) {
            TensorRef o = bld.alloc(m.out_c, h.H / 2, h.W / 2);     // 3x3 stride 2 pad 1 on even sizes
            ConvSpec cd{&h, nullptr, &o, m.wc, m.bc, m.sc};
            cd.stride = 2;
            if ((rc = bld.conv(cd))) return rc;
            h = o; g->outputs[m.name] = h;
        } else if ((rc = run_block(m))) return rc;
        skips.push_back(h);                                   // every down module pushes a skip (DDIMModel.py:232)
    }
    for (const Mod& m : p->mid) if ((rc = run_block(m))) return rc;
    const Mod* pending_up = nullptr;         // a ConvTranspose whose execution is deferred to its consumer
    auto flush_up = [&]() -> int {           // materialise the pending ConvTranspose for real
        if (!pending_up) return MI_OK;
        // the totals of its output come from chan_total_kernel, whose LDS grows with the width and is not raised past 64 KB
        const size_t tot_lds = chan_total_lds_bytes(pending_up->out_c);
        if (!tot_lds)
            return fail(MI_EINVAL, "%s: an unfolded ConvTranspose of %d channels: chan_total takes a multiple of 4 channels, at most 1024",
                        pending_up->name.c_str(), pending_up->out_c);
        if (tot_lds > CHAN_TOTAL_LDS_LIMIT)
            return fail(MI_EINVAL, "%s: an unfolded ConvTranspose of %d channels: chan_total needs %zu bytes of LDS for its output, the limit is %zu bytes",
                        pending_up->name.c_str(), pending_up->out_c, tot_lds, CHAN_TOTAL_LDS_LIMIT);
        TensorRef o = bld.alloc(pending_up->out_c, h.H * 2, h.W * 2);
        Op op{}; op.kind = OP_CONVT; op.s0 = h; op.dst = o; op.w = pending_up->wt; op.b = pending_up->bc;
        g->ops.push_back(op);
        bld.ensure_stats(o);
        g->outputs[pending_up->name] = o;
        h = o; pending_up = nullptr;
        return MI_OK;
    };
    for (const Mod& m : p->ups) {
        if (m.kind == MOD_UP) { if ((rc = flush_up())) return rc; pending_up = &m; continue; }
        if (m.kind == MOD_ATTN) { if ((rc = flush_up()) || (rc = run_block(m))) return rc; continue; }
        if (skips.empty()) return fail(MI_EINVAL, "%s: skip stack empty", m.name.c_str());
        TensorRef skip = skips.back(); skips.pop_back();          // only residual blocks pop (DDIMModel.py:240)
        if (pending_up) {
            if (skip.H == h.H && skip.W == h.W) {
                // ConvTranspose(4,2,1) then bilinear back to the skip's (half) size: one folded 3x3
                TensorRef o = bld.alloc(pending_up->out_c, h.H, h.W);
                ConvSpec cu{&h, nullptr, &o, pending_up->wc, pending_up->bc, pending_up->sc};
                cu.wide = true; cu.w_wide = pending_up->wcx;
                if ((rc = bld.conv(cu))) return rc;
                h = o; pending_up = nullptr;
            } else if ((rc = flush_up())) return rc;
        }
        if (h.H != skip.H || h.W != skip.W) {                      // F.interpolate(..., bilinear) (DDIMModel.py:241-242)
            TensorRef o = bld.alloc(h.C, skip.H, skip.W);
            bld.alloc_stats(o);                                    // the resize kernel leaves its own totals
            Op op{}; op.kind = OP_RESIZE; op.s0 = h; op.dst = o; g->ops.push_back(op);
            h = o;
        }
        TensorRef o; if ((rc = run_rb(m, h, &skip, &o))) return rc;
        h = o; g->outputs[m.name] = h;
    }
    if ((rc = flush_up())) return rc;
    if (h.H != H || h.W != W) return fail(MI_EINVAL, "network output is %dx%d for a %dx%d input", h.H, h.W, H, W);
    if ((rc = bld.gn_consumer(h, nullptr))) return rc;
    { Op o{}; o.kind = OP_OUT; o.s0 = h; o.gn = GnRef{p->g_out, p->be_out, true}; g->ops.push_back(o); }
    // every consumer is known: size the totals blocks, place the statistics arena, resolve the tensors' references
    size_t cur = 0;
    for (auto& st : bld.stats) {
        st.off = cur;
        cur += ((size_t)B * (st.C / st.bs) * g->stat_rep * STAT_WORDS * sizeof(stat_word) + 255) & ~(size_t)255;
    }
    g->stats_bytes = cur;
    g->stats_off = bld.take(g->stats_bytes);
    auto resolve = [&](TensorRef& t) {
        if (t.stat_id >= 0) { t.tot_off = g->stats_off + bld.stats[t.stat_id].off; t.stat_bs = bld.stats[t.stat_id].bs; }
    };
    for (Op& o : g->ops) for (TensorRef* t : {&o.s0, &o.s1, &o.dst, &o.resid, &o.res0, &o.res1}) resolve(*t);
    for (auto& kv : g->outputs) resolve(kv.second);
    g->bytes = (bld.cur + 255) & ~(size_t)255;
    return MI_OK;
}

// The program parameters that follow from (plan, B, side_by_side).
// side_by_side: the program runs next to another sub-batch's program on a second stream (mi_denoise split); its
// convs then ask for fewer persistent workgroups (640 instead of 768: each kernel has about half the chip; same-box
// A/B +2.5 % split, while an unsplit run loses 4 % with 640)
static void setup_program(const mi_plan* p, int B, bool side_by_side, Program* g) {
    g->persist_wgs = side_by_side ? 640 : 0;      // (same-box sweep in round 3: 512 .. 640 within 0.3 %, 448 and 704 .. 768 lose 1 %)
    // batch-invariant: the persistent workgroups PER SAMPLE (and with them the grouping of the statistics' partial
    // sums) must not depend on B or on the split: target / (B * ny) workgroups per sample with target = (640 / INVARIANT_B) B
    if (p->batch_invariant) g->persist_wgs = 640 / INVARIANT_B * B;
    // Wide 3x3 chunks (32 channels per chunk, 9 full K steps instead of 2 x 5, half the chunk hand-overs; 72-77 KB of LDS
    // per workgroup) on the launches of <= 512 workgroups: same-box A/B in round 3, B = 8 at 256x256: +2.3 % for a
    // program that runs alone, -3.5 % side by side (the other sub-batch's workgroups no longer fit beside them on a
    // CU) -- so only programs that run alone take them.  Not in batch-invariant plans: the K order is part of the bits.
    g->wide_chunks = !side_by_side && !p->batch_invariant;
}

static bool plan_as_side() {
    static const bool on = getenv("MIDD_PLAN_AS_SIDE") != nullptr;
    return on;
}

int midd::get_program(mi_plan* p, int B, int H, int W, Program** out, bool side_by_side) {
    if (!p->finalized) return fail(MI_ESTATE, "mi_unet_finalize has not been called (or weights changed since)");
    // development knob (tools/profile_round.sh): plan a program that runs alone exactly as a side-by-side sub-batch program is
    // planned, so that counter passes can measure the default run's launches without the other stream's traffic in their windows
    side_by_side = side_by_side || plan_as_side();
    const uint64_t key = ((uint64_t)(side_by_side ? 1 : 0) << 63) ^ ((uint64_t)B << 40) ^ ((uint64_t)H << 20) ^ (uint64_t)W;
    std::lock_guard<std::mutex> lk(p->mu);
    auto it = p->programs.find(key);
    if (it == p->programs.end()) {
        std::unique_ptr<Program> g(new Program());
        setup_program(p, B, side_by_side, g.get());
        int rc = build_program(p, B, H, W, g.get());
        if (rc) return rc;
        it = p->programs.emplace(key, std::move(g)).first;
    }
    *out = it->second.get();
    return MI_OK;
}

// number of independent sub-batches mi_denoise runs side by side (MIDD_SPLIT = 1 | 2 | 4; default 2)
int midd::split_parts(int B) {
    static const int want = getenv("MIDD_SPLIT") ? atoi(getenv("MIDD_SPLIT")) : 2;
    int parts = (want >= 4) ? 4 : (want >= 2 ? 2 : 1);
    while (parts > 1 && (B % parts || B / parts < 2)) parts /= 2;
    return parts;
}

// Workspace bytes of one forward / sampler run at batch B: the whole-batch program, or the sub-batch programs mi_denoise runs
// side by side when the batch splits.  The ONE place that knows this (mi_workspace_bytes, mi_ensemble_workspace_bytes).
// A finalized plan answers from its cached programs; an unfinalized one plans a throw-away program (host only, as
// mi_debug_plan_dump does).  0: unsupported shape (mi_last_error)
static size_t sampler_bytes(mi_plan* p, int B, int H, int W) {
    auto bytes_of = [&](int b, bool side) -> size_t {
        if (p->finalized) { Program* g = nullptr; return get_program(p, b, H, W, &g, side) ? 0 : g->bytes; }
        Program g;
        setup_program(p, b, side || plan_as_side(), &g);
        std::lock_guard<std::mutex> lk(p->mu);
        return build_program(p, b, H, W, &g) ? 0 : g.bytes;
    };
    size_t need = bytes_of(B, false);
    const int parts = split_parts(B);            // mi_denoise runs sub-batches side by side
    if (need && parts > 1) {
        const size_t part = bytes_of(B / parts, true);
        if (!part) return 0;
        if (parts * part > need) need = parts * part;
    }
    return need;
}

extern "C" size_t mi_workspace_bytes(mi_plan* plan, int B, int H, int W) {
    Program* g = nullptr;
    if (!plan || get_program(plan, B, H, W, &g)) return 0;      // (needs a finalized plan, as before)
    return sampler_bytes(plan, B, H, W);
}

int midd::ensemble_layout(mi_plan* p, int B, int members, int H, int W, int pass_samples, bool samples_external, EnsembleLayout* L) {
    auto round256 = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const int64_t V = (int64_t)B * members;
    L->pass = (int)(V < pass_samples ? V : pass_samples);
    if (L->pass > 65535) L->pass = 65535;                // "at most pass_samples": the broadcast kernel's grid holds this many
    L->tail = (int)(V % L->pass);
    L->run_bytes = sampler_bytes(p, L->pass, H, W);
    if (!L->run_bytes) return MI_EINVAL;                 // (mi_last_error holds the planner's message)
    if (L->tail) {                                       // (a smaller batch may plan wider tiles: take the larger of the two)
        const size_t t = sampler_bytes(p, L->tail, H, W);
        if (!t) return MI_EINVAL;
        if (t > L->run_bytes) L->run_bytes = t;
    }
    const size_t chw = (size_t)p->cfg.in_channels * H * W;
    L->cond_off = round256(L->run_bytes);
    L->samples_off = L->cond_off + round256((size_t)L->pass * chw * sizeof(float));
    L->bytes = L->samples_off + (samples_external ? 0 : (size_t)V * chw * sizeof(float));
    return MI_OK;
}

extern "C" size_t mi_ensemble_workspace_bytes(mi_plan* plan, int B, int members, int H, int W, int pass_samples, int samples_external) {
    if (check_ensemble_args(plan, B, members, H, W, 0, 0, pass_samples)) return 0;
    EnsembleLayout L{};
    if (ensemble_layout(plan, B, members, H, W, pass_samples, samples_external != 0, &L)) return 0;
    return L.bytes;
}

// (the layout depends on the NUMBER of views alone, so the list itself is not an argument)
extern "C" size_t mi_self_ensemble_workspace_bytes(mi_plan* plan, int B, int n_views, int H, int W, int pass_samples, int samples_external) {
    (void)samples_external;                              // the view-frame outputs always live in the workspace (include/midd.h)
    if (n_views < 1 || n_views > DIHEDRAL_MAX_VIEWS) {
        fail(MI_EINVAL, "n_views %d outside [1, %d]: a view list holds 1 to 8 distinct view codes (limit: 1 <= n_views <= %d)", n_views,
             DIHEDRAL_MAX_VIEWS, DIHEDRAL_MAX_VIEWS);
        return 0;
    }
    if (check_ensemble_args(plan, B, n_views, H, W, 0, 0, pass_samples)) return 0;
    EnsembleLayout L{};
    if (ensemble_layout(plan, B, n_views, H, W, pass_samples, false, &L)) return 0;
    return L.bytes;
}

extern "C" size_t mi_tiled_workspace_bytes(mi_plan* plan, int B, int H, int W, int th, int tw, int oy, int ox, int pass_samples, int tiles_external) {
    TileGeom g{};
    if (check_tiled_args(plan, B, H, W, th, tw, oy, ox, 0, pass_samples, &g)) return 0;
    EnsembleLayout L{};
    if (ensemble_layout(plan, B, g.ny * g.nx, th, tw, pass_samples, tiles_external != 0, &L)) return 0;
    return L.bytes;
}

int midd::tiled_ensemble_layout(mi_plan* p, int B, int members, int tiles, int th, int tw, int pass_samples, bool tiles_external, EnsembleLayout* L) {
    if (int rc = ensemble_layout(p, B, tiles, th, tw, pass_samples, true, L)) return rc;      // the passes of one member
    if (!tiles_external) L->bytes += (size_t)members * B * tiles * p->cfg.in_channels * th * tw * sizeof(float);
    return MI_OK;
}

extern "C" size_t mi_tiled_ensemble_workspace_bytes(mi_plan* plan, int B, int members, int H, int W, int th, int tw, int oy, int ox,
                                                    int pass_samples, int tiles_external) {
    TileGeom g{};
    if (check_tiled_ensemble_args(plan, B, members, H, W, th, tw, oy, ox, 0, 0, pass_samples, &g)) return 0;
    EnsembleLayout L{};
    if (tiled_ensemble_layout(plan, B, members, g.ny * g.nx, th, tw, pass_samples, tiles_external != 0, &L)) return 0;
    return L.bytes;
}

int midd::tiled_self_ensemble_layout(mi_plan* p, int B, int n_views, int tiles, int H, int W, int th, int tw, int pass_samples, bool tiles_external,
                                     EnsembleLayout* L, size_t* view_off) {
    if (int rc = ensemble_layout(p, B, tiles, th, tw, pass_samples, true, L)) return rc;      // the passes of one view
    const size_t C = (size_t)p->cfg.in_channels;
    *view_off = L->samples_off;
    L->samples_off += ((size_t)B * C * H * W * sizeof(float) + 255) & ~(size_t)255;
    L->bytes = L->samples_off + (tiles_external ? 0 : (size_t)n_views * B * tiles * C * th * tw * sizeof(float));
    return MI_OK;
}

int midd::tiled_fused_layout(mi_plan* p, int B, int tiles, int th, int tw, int pass_samples, bool tiles_external, EnsembleLayout* L) {
    if (int rc = ensemble_layout(p, B, tiles, th, tw, pass_samples, true, L)) return rc;      // the passes of one step
    const size_t all = (size_t)B * tiles * p->cfg.in_channels * th * tw * sizeof(float);
    L->samples_off = L->cond_off + ((all + 255) & ~(size_t)255);                              // the condition tiles of every pass stay
    L->bytes = L->samples_off + (tiles_external ? 0 : all);
    return MI_OK;
}

extern "C" size_t mi_tiled_fused_workspace_bytes(mi_plan* plan, int B, int H, int W, int th, int tw, int oy, int ox, int pass_samples, int tiles_external) {
    TileGeom g{};
    if (check_tiled_args(plan, B, H, W, th, tw, oy, ox, 0, pass_samples, &g)) return 0;
    EnsembleLayout L{};
    if (tiled_fused_layout(plan, B, g.ny * g.nx, th, tw, pass_samples, tiles_external != 0, &L)) return 0;
    return L.bytes;
}

// Kernel symbol + algorithmic work of one op (for mi_profile_*).
void midd::op_work(mi_plan* p, Program* g, const Op& o, std::string* name, double* flops, double* bytes) {
    const double B = g->B;
    char buf[128];
    auto elems = [&](const TensorRef& t) { return B * t.H * t.W * t.C; };
    switch (o.kind) {
        case OP_IN_CONV:
            *name = p->cfg.in_channels == 1 ? "midd::in_conv1_kernel" : "midd::in_conv_kernel";
            *flops = 2.0 * B * g->H * g->W * o.dst.C * 9 * 2 * p->cfg.in_channels;
            *bytes = 4.0 * (2.0 * B * p->cfg.in_channels * g->H * g->W + elems(o.dst));
            break;
        case OP_CHAN_TOT: *name = "midd::chan_total_kernel"; *flops = 0; *bytes = 4.0 * elems(o.s0); break;
        case OP_CONV: {
            // the kernel that really runs: "f16x3" = two planes / three products, "f16" = one plane / one product
            const char* mode = p->cfg.compute_mode == MI_COMPUTE_F16X3 ? "f16x3" : p->cfg.compute_mode == MI_COMPUTE_F16 ? "f16" : "f32";
            if (fp16_mfma(p->cfg) && o.tile.ks == 1 && o.tile.tw == 0)
                snprintf(buf, sizeof(buf), "midd::conv1x1_%s_kernel<%d, %d, %d>", mode, o.tile.mt, o.tile.nt, o.att_mode);
            else {
                char tail[32] = "";         // fp16 MFMA: the RES flag and the chunk width (template arguments 8 and 9)
                if (fp16_mfma(p->cfg))
                    snprintf(tail, sizeof(tail), ", %s, %d", (o.res_steps > 0 && o.tile.stride == 1 && o.tile.ks == 3) ? "true" : "false", o.tile.cb);
                snprintf(buf, sizeof(buf), "midd::conv_mfma_%s_kernel<%d, %d, %d, %d, %d, %d, %d%s>",
                         mode, o.tile.ks, o.tile.stride,
                         o.tile.tw, o.tile.mt, o.tile.nt, o.tile.wm, o.tile.wn, tail);
            }
            *name = buf;
            const double cin = o.s0.C + (o.has_s1 ? o.s1.C : 0);
            const double res_cin = o.res_steps > 0 ? o.res0.C + (o.has_res1 ? o.res1.C : 0) : 0;      // folded res_conv (1x1 over the block input)
            *flops = 2.0 * elems(o.dst) * (cin * o.ks * o.ks + res_cin);
            *bytes = 4.0 * (elems(o.s0) + (o.has_s1 ? elems(o.s1) : 0) + elems(o.dst) + (o.has_resid ? elems(o.resid) : 0)
                            + (o.res_steps > 0 ? elems(o.res0) + (o.has_res1 ? elems(o.res1) : 0) : 0)
                            + (double)o.dst.C * (cin * o.ks * o.ks + res_cin));
            break;
        }
        case OP_ATTN: {
            const double N = (double)o.dst.H * o.dst.W;
            snprintf(buf, sizeof(buf), "midd::attention_%s_kernel<%d>", p->cfg.compute_mode == MI_COMPUTE_F16X3 ? "f16x3" : p->cfg.compute_mode == MI_COMPUTE_F16 ? "f16" : "f32", o.dst.C / 2);
            *name = buf;
            *flops = 4.0 * B * N * N * o.dst.C;              // QK^T + PV over both heads
            *bytes = 4.0 * (elems(o.s0) + elems(o.dst));
            break;
        }
        case OP_RESIZE: *name = "midd::resize_bilinear_kernel"; *flops = 0; *bytes = 4.0 * (elems(o.s0) + elems(o.dst)); break;
        case OP_CONVT:
            *name = "midd::conv_transpose_kernel";
            *flops = 2.0 * elems(o.s0) * o.dst.C * 16; *bytes = 4.0 * (elems(o.s0) + elems(o.dst));
            break;
        case OP_OUT:
            *name = p->cfg.in_channels == 1 ? "midd::out_conv_kernel<1>" : "midd::out_conv_kernel<0>";
            *flops = 2.0 * B * g->H * g->W * o.s0.C * 9 * p->cfg.in_channels;
            *bytes = 4.0 * (elems(o.s0) + 3.0 * B * p->cfg.in_channels * g->H * g->W);
            break;
    }
}

// Debug/test hook, host only: the execution program the planner builds for (B, H, W) -- one line per launch with its tile,
// grid, persistent workgroups, ring depth / DMA pieces, res steps, key split and LDS bytes.  side_by_side: as a sub-batch
// program of the two-stream run is planned.  Needs no finalize (weight offsets print as 0).  Returns the text length.
int midd::dump_program(mi_plan* p, int B, int H, int W, bool side_by_side, std::string* out) {
    Program g;
    setup_program(p, B, side_by_side, &g);
    auto appendf = [out](const char* fmt, auto... v) {      // formats straight into the text, whatever the length
        const size_t at = out->size(), n = snprintf(nullptr, 0, fmt, v...);
        out->resize(at + n + 1);
        snprintf(&(*out)[at], n + 1, fmt, v...);
        out->resize(at + n);
    };
    {
        std::lock_guard<std::mutex> lk(p->mu);       // the topology's weight offsets and scales change under finalize
        if (int rc = build_program(p, B, H, W, &g)) return rc;
    }
    appendf("program B=%d %dx%d side=%d bytes=%zu stats_off=%zu stats_bytes=%zu stat_rep=%d persist_wgs=%d wide=%d ops=%zu\n",
            B, H, W, (int)side_by_side, g.bytes, g.stats_off, g.stats_bytes, g.stat_rep, g.persist_wgs, (int)g.wide_chunks, g.ops.size());
    static const char* kinds[] = {"in_conv", "conv", "attn", "resize", "convT", "out", "chan_tot"};
    for (const Op& o : g.ops) {
        std::string name; double fl, by;
        op_work(p, &g, o, &name, &fl, &by);
        appendf("op%03d %-8s %dx%d c%d+%d->%d k%d s%d pro%d res_steps%d att%d ksplit%d tps%d bs(in %d,%d out %d) | %s",
                (int)(&o - g.ops.data()), kinds[o.kind], o.dst.H ? o.dst.H : H, o.dst.W ? o.dst.W : W, o.s0.C, o.has_s1 ? o.s1.C : 0, o.dst.C, o.ks, o.stride,
                o.prologue, o.res_steps, o.att_mode, o.att_ksplit, o.att_tps, o.s0.stat_bs, o.has_s1 ? o.s1.stat_bs : 0, o.dst.stat_bs, name.c_str());
        ConvLaunchInfo li{};
        if (o.kind == OP_CONV && fp16_mfma(p->cfg) &&
            conv16_launch_info(o.s0.C + (o.has_s1 ? o.s1.C : 0), o.dst.C, B, o.dst.H, o.dst.W, o.tile, g.persist_wgs, &li))
            appendf(" | grid %dx%d wgs/img %d tiles %dx%d ring %d ppw %d apw %d lds %d", li.grid_x, li.grid_y, li.wgs_per_img,
                    li.tiles_x, li.tiles_y, li.ring, li.ppw, li.apw, li.lds_bytes);
        *out += '\n';
    }
    return MI_OK;
}
