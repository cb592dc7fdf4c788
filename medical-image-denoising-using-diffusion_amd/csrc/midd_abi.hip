// C ABI surface of libmidd.so (include/midd.h): error state, version, plan create / destroy, weight loading, status word,
// and the thin wrappers of the pre/post-processing kernels (prepost.hip) and of the debug hooks.
//
// Reference interfaces replaced (cited per function in the units that implement them):
//   UNetDiffusion.__init__ / forward   Backend/DDIM/DDIMModel.py:169-248
//   DiffusionDenoiser.denoise          Backend/DDIM/DDIMModel.py:268-289
//   cddpm variants                     Backend/cddpm/cddpmModels.py:176-308
#include "midd_host.h"

using namespace midd;

// ------------------------------------------------------------------------------ errors
static thread_local char g_err[512] = "";

int midd::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

// ------------------------------------------------------------------------------ C ABI: pre/post-processing
extern "C" size_t mi_resize_workspace_bytes(int n, int sw, int sh, int dw, int dh) {
    if (n < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1) return 0;
    return resize_workspace_bytes(n, sw, sh, dw, dh);
}
extern "C" int mi_resize_bicubic_u8(const void* src, int n, int sw, int sh, void* dst, int dw, int dh,
                                    void* workspace, size_t workspace_bytes, void* stream) {
    if (!src || !dst || !workspace) return fail(MI_EINVAL, "null argument");
    if (n < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1) return fail(MI_EINVAL, "image sizes must be positive");
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(MI_EINVAL, "workspace must be 256-byte aligned");
    if (workspace_bytes < resize_workspace_bytes(n, sw, sh, dw, dh))
        return fail(MI_EINVAL, "workspace too small: %zu < %zu", workspace_bytes, resize_workspace_bytes(n, sw, sh, dw, dh));
    HIPCHK(resize_bicubic_u8_launch(static_cast<const unsigned char*>(src), n, sw, sh, static_cast<unsigned char*>(dst), dw, dh,
                                    workspace, static_cast<hipStream_t>(stream)));
    return MI_OK;
}
extern "C" int mi_u8_to_unit_f32(const void* src, void* dst, size_t count, void* stream) {
    if (!src || !dst) return fail(MI_EINVAL, "null argument");
    HIPCHK(u8_to_unit_launch(static_cast<const unsigned char*>(src), static_cast<float*>(dst), count, static_cast<hipStream_t>(stream)));
    return MI_OK;
}
extern "C" int mi_unit_f32_to_u8(const void* src, void* dst, size_t count, void* stream) {
    if (!src || !dst) return fail(MI_EINVAL, "null argument");
    HIPCHK(unit_to_u8_launch(static_cast<const float*>(src), static_cast<unsigned char*>(dst), count, static_cast<hipStream_t>(stream)));
    return MI_OK;
}
// n * h * w of the source, the intermediate and the destination stay below 2^31 (one thread per element, 32-bit grid)
static bool resize_f32_fits(int n, int sw, int sh, int dw, int dh) {
    const long long lim = 1LL << 31;
    return (long long)n * sh * sw < lim && (long long)n * sh * dw < lim && (long long)n * dh * dw < lim;
}
extern "C" size_t mi_resize_f32_workspace_bytes(int n, int sw, int sh, int dw, int dh) {
    if (n < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1 || !resize_f32_fits(n, sw, sh, dw, dh)) return 0;
    return resize_f32_workspace_bytes(n, sw, sh, dw, dh);
}
// the argument rules shared by mi_resize_bicubic_f32 and its windowed form
static int resize_f32_args(const void* src, int src_type, int n, int sw, int sh, void* dst, int dst_type, int dw, int dh,
                           void* workspace, size_t workspace_bytes) {
    if (!src || !dst || !workspace) return fail(MI_EINVAL, "null argument");
    if (n < 1 || sw < 1 || sh < 1 || dw < 1 || dh < 1) return fail(MI_EINVAL, "image sizes must be positive");
    if (src_type != MI_PIX_U8 && src_type != MI_PIX_U16 && src_type != MI_PIX_F32)
        return fail(MI_EINVAL, "unknown source element type %d (MI_PIX_U8, MI_PIX_U16 or MI_PIX_F32)", src_type);
    if (dst_type == MI_PIX_U8)
        return fail(MI_EINVAL, "destination element type MI_PIX_U8: the 8-bit destination is mi_resize_bicubic_u8 (fixed-point arithmetic)");
    if (dst_type != MI_PIX_U16 && dst_type != MI_PIX_F32)
        return fail(MI_EINVAL, "unknown destination element type %d (MI_PIX_U16 or MI_PIX_F32)", dst_type);
    if (!resize_f32_fits(n, sw, sh, dw, dh)) return fail(MI_EINVAL, "too many pixels: n * height * width must stay below 2^31");
    if (reinterpret_cast<uintptr_t>(workspace) & 255) return fail(MI_EINVAL, "workspace must be 256-byte aligned");
    if (workspace_bytes < resize_f32_workspace_bytes(n, sw, sh, dw, dh))
        return fail(MI_EINVAL, "workspace too small: %zu < %zu", workspace_bytes, resize_f32_workspace_bytes(n, sw, sh, dw, dh));
    return MI_OK;
}
extern "C" int mi_resize_bicubic_f32(const void* src, int src_type, int n, int sw, int sh, void* dst, int dst_type, int dw, int dh,
                                     int clamp01, void* workspace, size_t workspace_bytes, void* stream) {
    if (const int rc = resize_f32_args(src, src_type, n, sw, sh, dst, dst_type, dw, dh, workspace, workspace_bytes)) return rc;
    HIPCHK(resize_bicubic_f32_launch(src, src_type, n, sw, sh, dst, dst_type, dw, dh, clamp01, workspace, static_cast<hipStream_t>(stream)));
    return MI_OK;
}
extern "C" int mi_u16_to_unit_f32(const uint16_t* src, float* dst, size_t count, void* stream) {
    if (!src || !dst) return fail(MI_EINVAL, "null argument");
    if (count >= ((size_t)1 << 40)) return fail(MI_EINVAL, "count must stay below 2^40");
    HIPCHK(u16_to_unit_launch(src, dst, count, static_cast<hipStream_t>(stream)));
    return MI_OK;
}
extern "C" int mi_unit_f32_to_u16(const float* src, uint16_t* dst, size_t count, void* stream) {
    if (!src || !dst) return fail(MI_EINVAL, "null argument");
    if (count >= ((size_t)1 << 40)) return fail(MI_EINVAL, "count must stay below 2^40");
    HIPCHK(unit_to_u16_launch(src, dst, count, static_cast<hipStream_t>(stream)));
    return MI_OK;
}
// ---- the window (include/midd.h: THE WINDOW)
static int window_counts(int n, size_t count) {
    if (n < 1 || n > 65535) return fail(MI_EINVAL, "n must be in [1, 65535], got %d", n);
    if (count < 1 || count > 0xffffffffull) return fail(MI_EINVAL, "count must be in [1, 2^32), got %zu", count);
    return MI_OK;
}
extern "C" int mi_histogram_u16(const uint16_t* src, int n, size_t count, uint32_t* hist, void* stream) {
    if (!src || !hist) return fail(MI_EINVAL, "null argument");
    if (const int rc = window_counts(n, count)) return rc;
    if (reinterpret_cast<uintptr_t>(src) & 1) return fail(MI_EINVAL, "src must be 2-byte aligned");
    if (reinterpret_cast<uintptr_t>(hist) & 15) return fail(MI_EINVAL, "hist must be 16-byte aligned");
    HIPCHK(histogram_u16_launch(src, n, count, hist, static_cast<hipStream_t>(stream)));
    return MI_OK;
}
extern "C" int mi_window_levels(const uint32_t* hist, int n, double p_lo, double p_hi, int32_t* levels, void* stream) {
    if (!hist || !levels) return fail(MI_EINVAL, "null argument");
    if (n < 1 || n > 65535) return fail(MI_EINVAL, "n must be in [1, 65535], got %d", n);
    if (!std::isfinite(p_lo) || !std::isfinite(p_hi)) return fail(MI_EINVAL, "percentiles must be finite");
    if (!(0.0 <= p_lo && p_lo < p_hi && p_hi <= 100.0))
        return fail(MI_EINVAL, "percentiles must satisfy 0 <= p_lo < p_hi <= 100, got (%g, %g)", p_lo, p_hi);
    if (reinterpret_cast<uintptr_t>(hist) & 15) return fail(MI_EINVAL, "hist must be 16-byte aligned");
    HIPCHK(window_levels_launch(hist, n, p_lo, p_hi, levels, static_cast<hipStream_t>(stream)));
    return MI_OK;
}
extern "C" int mi_window_u16_to_f32(const uint16_t* src, const int32_t* levels, int n, size_t count, float* dst, void* stream) {
    if (!src || !levels || !dst) return fail(MI_EINVAL, "null argument");
    if (const int rc = window_counts(n, count)) return rc;
    HIPCHK(window_u16_to_f32_launch(src, levels, n, count, dst, static_cast<hipStream_t>(stream)));
    return MI_OK;
}
extern "C" int mi_window_f32_to_u16(const float* src, const int32_t* levels, int n, size_t count, uint16_t* dst, void* stream) {
    if (!src || !levels || !dst) return fail(MI_EINVAL, "null argument");
    if (const int rc = window_counts(n, count)) return rc;
    HIPCHK(window_f32_to_u16_launch(src, levels, n, count, dst, static_cast<hipStream_t>(stream)));
    return MI_OK;
}
extern "C" int mi_resize_bicubic_f32_window(const void* src, int src_type, int n, int sw, int sh, void* dst, int dst_type, int dw, int dh,
                                            int clamp01, const int32_t* levels, void* workspace, size_t workspace_bytes, void* stream) {
    if (!levels) return mi_resize_bicubic_f32(src, src_type, n, sw, sh, dst, dst_type, dw, dh, clamp01, workspace, workspace_bytes, stream);
    if (const int rc = resize_f32_args(src, src_type, n, sw, sh, dst, dst_type, dw, dh, workspace, workspace_bytes)) return rc;
    if (n > 65535) return fail(MI_EINVAL, "n must be in [1, 65535] under a window, got %d", n);
    if (src_type != MI_PIX_U16 && dst_type != MI_PIX_U16)
        return fail(MI_EINVAL, "levels given, but neither side is MI_PIX_U16: the window acts on 16-bit elements only");
    HIPCHK(resize_bicubic_f32_window_launch(src, src_type, n, sw, sh, dst, dst_type, dw, dh, clamp01, levels, workspace,
                                            static_cast<hipStream_t>(stream)));
    return MI_OK;
}
extern "C" size_t mi_metrics_workspace_bytes(int n, int h) { return (n < 1 || h < 1) ? 0 : metrics_workspace_bytes(n, h); }
extern "C" int mi_image_metrics(const void* target, const void* pred, int n, int h, int w, void* out,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (!target || !pred || !out || !workspace) return fail(MI_EINVAL, "null argument");
    if (n < 1 || h < 7 || w < 7) return fail(MI_EINVAL, "images must be at least 7x7 (SSIM window), got %dx%d", h, w);
    if (workspace_bytes < metrics_workspace_bytes(n, h)) return fail(MI_EINVAL, "workspace too small");
    HIPCHK(metrics_launch(static_cast<const float*>(target), static_cast<const float*>(pred), n, h, w, static_cast<double*>(out),
                          workspace, static_cast<hipStream_t>(stream)));
    return MI_OK;
}

// ------------------------------------------------------------------------------ C ABI: create / load
extern "C" const char* mi_last_error(void) { return g_err; }
extern "C" const char* mi_version(void) { return "midd 0.4 gfx950 (fp32 MFMA | split-fp16 x3 MFMA | fp16 MFMA; GroupNorm statistics in the producers; device pre/post-processing)"; }

#ifndef MIDD_SOURCE_HASH
#define MIDD_SOURCE_HASH "unknown"
#endif
extern "C" const char* mi_source_hash(void) { return MIDD_SOURCE_HASH; }

extern "C" int mi_debug_attention_split(int N, int B, int* ksplit, int* tiles_per_split) {
    if (N < 1 || B < 1 || !ksplit || !tiles_per_split) return fail(MI_EINVAL, "N and B must be positive");
    attention16_split(N, ATTN_HEADS_ABI, B, ksplit, tiles_per_split);
    return MI_OK;
}

extern "C" int mi_unet_plan_create(const mi_unet_cfg* cfg, mi_plan** out) {
    if (!cfg || !out) return fail(MI_EINVAL, "null argument");
    if (cfg->num_levels < 1 || cfg->num_levels > MI_MAX_LEVELS) return fail(MI_EINVAL, "num_levels out of range");
    if (cfg->num_attention_levels < 0 || cfg->num_attention_levels > MI_MAX_LEVELS) return fail(MI_EINVAL, "num_attention_levels out of range");
    if (cfg->model_channels < 16 || cfg->model_channels % 16) return fail(MI_EINVAL, "model_channels must be a multiple of 16 (MFMA K-chunk), got %d", cfg->model_channels);
    if (cfg->in_channels < 1 || cfg->in_channels > 4) return fail(MI_EINVAL, "in_channels must be 1..4");
    if (cfg->num_res_blocks < 1) return fail(MI_EINVAL, "num_res_blocks must be >= 1");
    if (cfg->time_emb_dim < 1) return fail(MI_EINVAL, "time_emb_dim must be >= 1");
    if (cfg->variant != MI_VARIANT_DDIM && cfg->variant != MI_VARIANT_CDDPM) return fail(MI_EINVAL, "unknown variant %d", cfg->variant);
    const int arith = cfg->compute_mode & ~MI_COMPUTE_BATCH_INVARIANT;
    if (arith != MI_COMPUTE_F32 && arith != MI_COMPUTE_F16X3 && arith != MI_COMPUTE_F16) return fail(MI_EINVAL, "unknown compute_mode %d", cfg->compute_mode);
    for (int i = 0; i < cfg->num_levels; ++i)
        if (cfg->channel_mult[i] < 1) return fail(MI_EINVAL, "channel_mult[%d] must be >= 1", i);
    // The two pointwise kernels at the ends of the network keep their weights in LDS: a width whose launch would be refused is
    // refused here, with the limit named (the sizes are the launches' own: midd_internal.h).  in_conv's width is model_channels,
    // out_conv's input is the last module of level 0 (build_topology: final_c = model_channels * channel_mult[0])
    {
        const int ic = cfg->in_channels, mc = cfg->model_channels;
        const long long fc = (long long)mc * cfg->channel_mult[0];
        if (mc > (1 << 20)) return fail(MI_EINVAL, "model_channels %d is out of range", mc);      // (the byte counts below stay inside an int)
        if (!(ic == 1 && in_conv1_width(mc)) && in_conv_lds_bytes(ic, mc) > POINTWISE_LDS_LIMIT)
            return fail(MI_EINVAL, "in_channels %d with model_channels %d: in_conv needs %zu bytes of LDS, the limit is %zu bytes",
                        ic, mc, in_conv_lds_bytes(ic, mc), POINTWISE_LDS_LIMIT);
        if (fc > (1 << 20) || out_conv_lds_bytes(ic, (int)fc) > POINTWISE_LDS_LIMIT)
            return fail(MI_EINVAL, "in_channels %d with %lld channels into out_conv (model_channels * channel_mult[0]): out_conv needs more than the "
                        "limit of %zu bytes of LDS (%zu bytes of tile, %d bytes per channel)",
                        ic, fc, POINTWISE_LDS_LIMIT, out_conv_static_lds_bytes(), (int)out_conv_dynamic_lds_bytes(ic, 1));
    }
    for (int i = 0; i < cfg->num_attention_levels; ++i) {
        const int lv = cfg->attention_levels[i];
        if (lv >= 0 && lv < cfg->num_levels) {
            const int c = cfg->model_channels * cfg->channel_mult[lv];
            if (c % ATTN_HEADS_ABI || !attention_supported(c / 2))
                return fail(MI_EINVAL, "attention head_dim %d unsupported (32/64/96/128)", c / 2);
        }
    }
    std::unique_ptr<mi_plan> p(new mi_plan());
    p->cfg = *cfg;
    p->cfg.compute_mode = arith;
    p->batch_invariant = (cfg->compute_mode & MI_COMPUTE_BATCH_INVARIANT) != 0;
    int rc = build_topology(p.get());
    if (rc) return rc;
    *out = p.release();
    return MI_OK;
}

extern "C" int mi_unet_num_weights(const mi_plan* plan) { return plan ? (int)plan->expected.size() : 0; }
extern "C" const char* mi_unet_weight_name(const mi_plan* plan, int i) {
    if (!plan || i < 0 || i >= (int)plan->expected.size()) return nullptr;
    return plan->expected[i].c_str();
}

extern "C" int mi_unet_load_weights(mi_plan* plan, const char* key, const float* data, const int64_t* shape, int ndim) {
    if (!plan || !key || !data || !shape) return fail(MI_EINVAL, "null argument");
    auto it = plan->expected_shape.find(key);
    if (it == plan->expected_shape.end()) return fail(MI_EINVAL, "unexpected key in state_dict: \"%s\"", key);
    const std::vector<int64_t>& want = it->second;
    bool ok = (int)want.size() == ndim;
    for (int i = 0; ok && i < ndim; ++i) ok = want[i] == shape[i];
    if (!ok) return fail(MI_EINVAL, "size mismatch for %s", key);
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) n *= (size_t)shape[i];
    std::lock_guard<std::mutex> lk(plan->mu);
    HostWeight& hw = plan->host[key];
    hw.shape.assign(shape, shape + ndim);
    hw.data.assign(data, data + n);
    hw.loaded = true;
    plan->finalized = false;
    return MI_OK;
}

extern "C" int mi_status(const void* workspace, void* stream, int* flags) {
    if (!workspace || !flags) return fail(MI_EINVAL, "null argument");
    int host = 0;
    HIPCHK(hipMemcpyAsync(&host, workspace, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
    HIPCHK(hipStreamSynchronize((hipStream_t)stream));
    *flags = host;
    // diagnostic builds (-DMIDD_DMA_CHECK): the NaN sentinel of a transfer that had not landed also sets the other two bits
    if (host & ~(MI_STATUS_NONFINITE | MI_STATUS_FP16_RANGE))
        return fail(MI_ERANGE, "status word 0x%x (bit 4: a -DMIDD_DMA_CHECK build saw an operand that had not landed when its counted wait returned)", host);
    // the range flag first: an operand beyond fp16 turns into Inf / NaN downstream, so both bits are usually set then
    if (host & MI_STATUS_FP16_RANGE)
        return fail(MI_ERANGE, "an attention operand exceeds the split-fp16 range (|q|, |k| or |v| >= 4094, or not finite): use compute=\"f32\"%s",
                    (host & MI_STATUS_NONFINITE) ? "; non-finite values, or finite ones beyond the statistics range, reached GroupNorm statistics" : "");
    // (the same bit for both: a finite partial sum of squares >= 2^59 adds the sentinel an Inf / NaN partial adds, stats_common.h)
    if (host & MI_STATUS_NONFINITE)
        return fail(MI_ERANGE, "non-finite activations (NaN / Inf), or finite ones beyond the statistics range (a workgroup's sum of squares of one "
                               "channel >= 2^59; midd.h: MI_STATUS_NONFINITE), reached a GroupNorm statistic or a raw operand");
    return MI_OK;
}

extern "C" int mi_debug_conv16_geometry(int ks, int stride, int tw, int mt, int nt, int wm, int wn, int cb, int* ring, int* ppw, int* apw, int* lds_bytes) {
    if (!ring || !ppw || !apw || !lds_bytes) return fail(MI_EINVAL, "null argument");
    ConvTile t{ks, stride, tw, mt, nt, wm, wn, cb};
    ConvLaunchInfo li{};
    if (!conv16_launch_info(384, 16 * nt * wn, 1, 64, 64, t, 0, &li)) return fail(MI_EINVAL, "tile (%d,%d,%d,%d,%d) ks %d stride %d cb %d is not instantiated", tw, mt, nt, wm, wn, ks, stride, cb);
    *ring = li.ring; *ppw = li.ppw; *apw = li.apw; *lds_bytes = li.lds_bytes;
    return MI_OK;
}
extern "C" int mi_debug_conv16_geometry_planes(int ks, int stride, int tw, int mt, int nt, int wm, int wn, int cb, int planes,
                                               int* ring, int* ppw, int* apw, int* lds_bytes) {
    if (!ring || !ppw || !apw || !lds_bytes) return fail(MI_EINVAL, "null argument");
    if (planes != 1 && planes != 2) return fail(MI_EINVAL, "planes must be 1 (f16) or 2 (f16x3), got %d", planes);
    ConvTile t{ks, stride, tw, mt, nt, wm, wn, cb, planes};
    ConvLaunchInfo li{};
    if (!conv16_launch_info(384, 16 * nt * wn, 1, 64, 64, t, 0, &li)) return fail(MI_EINVAL, "tile (%d,%d,%d,%d,%d) ks %d stride %d cb %d is not instantiated", tw, mt, nt, wm, wn, ks, stride, cb);
    *ring = li.ring; *ppw = li.ppw; *apw = li.apw; *lds_bytes = li.lds_bytes;
    return MI_OK;
}
extern "C" int mi_debug_conv16_steps(int Cin, int ks, int cb) {
    if (Cin < 16 || Cin % 16) return fail(MI_EINVAL, "Cin %d: a positive multiple of 16", Cin);
    if (ks != 1 && ks != 3) return fail(MI_EINVAL, "ks %d: 1 or 3", ks);
    if (cb < 0 || cb > 2 || (ks == 1 && cb == 1)) return fail(MI_EINVAL, "cb %d: 0 (default), 1 (3x3) or 2", cb);
    return conv16_num_steps(Cin, ks * ks, cb);
}
extern "C" int mi_debug_plan_dump(mi_plan* plan, int B, int H, int W, int side_by_side, char* buf, size_t cap) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    std::string text;
    int rc = dump_program(plan, B, H, W, side_by_side != 0, &text);
    if (rc) return rc;
    if (buf && cap) { snprintf(buf, cap, "%s", text.c_str()); }
    return (int)text.size();
}

extern "C" void mi_plan_destroy(mi_plan* plan) {
    if (!plan) return;
    for (auto& sp : plan->spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    for (hipEvent_t ev : plan->event_pool) (void)hipEventDestroy(ev);
    if (plan->sev_fork) (void)hipEventDestroy(plan->sev_fork);
    for (int i = 0; i < mi_plan::MAX_PARTS; ++i) {
        if (plan->sev_phase[i]) (void)hipEventDestroy(plan->sev_phase[i]);
        if (plan->sev_join[i]) (void)hipEventDestroy(plan->sev_join[i]);
        if (plan->sstream[i]) (void)hipStreamDestroy(plan->sstream[i]);
    }
    if (plan->wdev) (void)hipFree(plan->wdev);
    if (plan->ttab) (void)hipFree(plan->ttab);
    delete plan;
}
