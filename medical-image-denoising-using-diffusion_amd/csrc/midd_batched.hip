// The batched sampler calls (virtual samples in passes: ensembles, tiles, tiled ensembles, flip / rotate views), their member /
// tile / view argument rules, and the stand-alone tile and dihedral calls they compose (reduce and quantiles: midd_analysis.hip).
#include "midd_sampler.h"
#include "tile_geometry.h"

using namespace midd;

// ---------------------------------------------------------------------------- ensembles of the stochastic sampler
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

// The one pass loop.  Round m (a member of the tiled ensemble or a view of the tiled self-ensemble, whose member word is a launch
// constant; else the only round) runs the virtual samples [0, V) in passes: fill(cond, m, v0, n) writes the pass's condition
// images, the sampler loop leaves its samples at store[m][v0 ..].  noise(m) is the round's StepNoise: the member word, and for
// tiles the whole-image frame, may differ from round to round (member_rounds: the member word alone does).  The caller holds
// plan->side_mu and has cleared the status word, so the word accumulates over the passes; every pass joins its side streams before
// it returns, on success and on failure (enqueue_run), and the first failing pass ends the call.
template <class Fill, class Noise>
static int run_passes(mi_plan* plan, Fill fill, float* store, int64_t V, int rounds, int h, int w, size_t chw, const EnsembleLayout& L,
                      Noise noise, const Schedule& sc, int flags, char* ws, void* stream) {
    float* cond = reinterpret_cast<float*>(ws + L.cond_off);
    for (int m = 0; m < rounds; ++m) {
        StepNoise sn = noise(m);
        for (int64_t v0 = 0; v0 < V; v0 += L.pass) {
            const int n = (int)(V - v0 < L.pass ? V - v0 : L.pass);
            if (int rc = fill(cond, m, (int)v0, n)) return rc;
            sn.v0 = (int)v0;
            Program* g = nullptr;
            float* x = store + ((size_t)m * V + (size_t)v0) * chw;
            if (int rc = check_run(plan, cond, x, n, h, w, sc, ws, L.run_bytes, &g)) return rc;
            if (int rc = enqueue_run(plan, g, cond, x, n, h, w, sc, nullptr, sn, flags, ws, L.run_bytes, stream)) return rc;
        }
    }
    return MI_OK;
}

// the rounds of a member-outer call (and the single round of the others): round m draws member word member_offset + m, nothing else changes
static auto member_rounds(const StepNoise& sn) {
    return [sn](int m) { StepNoise r = sn; r.member_offset = sn.member_offset + (uint32_t)m; return r; };
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
    auto broadcast = [&](float* cond, int, int v0, int n) { return launched(ensemble_broadcast_launch(noisy, cond, v0, n, members, chw, s), "ensemble_broadcast"); };
    if (int rc = run_passes(plan, broadcast, samples, (int64_t)B * members, 1, H, W, chw, L, member_rounds(sn), sc, flags, ws, stream)) return rc;
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

// what the stand-alone tile calls open with: the channels, the geometry, the tiles of the batch (mi_tile_extract: these three) ...
static int check_tile_shape(int B, int C, int H, int W, int th, int tw, int oy, int ox, TileGeom* g) {
    if (C < 1) return fail(MI_EINVAL, "C %d must be positive", C);
    if (int rc = fill_tile_geom(C, H, W, th, tw, oy, ox, g)) return rc;
    return check_tile_count(B, *g);
}
// ... and, where whole images are written, the elements of one (the three blend calls)
static int check_tile_run(int B, int C, int H, int W, int th, int tw, int oy, int ox, TileGeom* g) {
    if (int rc = check_tile_shape(B, C, H, W, th, tw, oy, ox, g)) return rc;
    return check_step_noise_range(C, H, W, 0);
}

extern "C" int mi_tile_extract(const float* noisy, int B, int C, int H, int W, int th, int tw, int oy, int ox, int v0, int n,
                               float* dst, void* stream) {
    TileGeom g{};
    if (int rc = check_tile_shape(B, C, H, W, th, tw, oy, ox, &g)) return rc;
    if (v0 < 0 || n < 0 || n > 65535 || (int64_t)v0 + n > (int64_t)B * g.ny * g.nx)
        return fail(MI_EINVAL, "tiles [%d, %d + %d) outside the %d * %d * %d tiles of the batch (limit per call: n <= 65535)", v0, v0, n, B, g.ny, g.nx);
    if ((int64_t)C * th * tw > 2147483647ll) return fail(MI_EINVAL, "C*th*tw = %d*%d*%d exceeds 2^31 - 1", C, th, tw);
    if (n == 0) return MI_OK;
    if (!noisy || !dst) return fail(MI_EINVAL, "null argument");
    return launched(tile_extract_launch(noisy, dst, g, v0, n, (hipStream_t)stream), "tile_extract");
}

extern "C" int mi_tile_blend(const float* tiles, int B, int C, int H, int W, int th, int tw, int oy, int ox, float* out, void* stream) {
    TileGeom g{};
    if (int rc = check_tile_run(B, C, H, W, th, tw, oy, ox, &g)) return rc;
    if (!tiles || !out) return fail(MI_EINVAL, "null argument");
    return launched(tile_blend_launch(tiles, out, B, g, (hipStream_t)stream), "tile_blend");
}

// mi_denoise_tiled_rule and mi_denoise_tiled_dpm behind their rules: `sc` carries the rule.  MI_UPDATE_DPMPP2M: sc.x0 is the call's x0_hist
// [pass_samples, C, th, tw], the in-place history of whichever pass runs
static int tiled_run(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out,
                     int B, int H, int W, int th, int tw, int oy, int ox, const Schedule& sc,
                     int seeded, uint64_t seed, int64_t sample_offset, int pass_samples, int flags,
                     void* workspace, size_t workspace_bytes, void* stream) {
    TileGeom tg{};
    if (int rc = check_tiled_args(plan, B, H, W, th, tw, oy, ox, sample_offset, pass_samples, &tg)) return rc;
    const int K = tg.ny * tg.nx;
    const size_t chw = (size_t)tg.C * th * tw, img = (size_t)tg.C * H * W * sizeof(float);
    const bool dpm = sc.rule == MI_UPDATE_DPMPP2M;
    if (dpm && sc.n > 0 && !sc.x0) return fail(MI_EINVAL, "null argument");
    const Buf buf[4] = {{noisy, (size_t)B * img, "noisy"}, {image_out, (size_t)B * img, "image_out"},
                        {tiles_out, (size_t)B * K * chw * sizeof(float), "tiles_out"},
                        {dpm ? sc.x0 : nullptr, (size_t)pass_samples * chw * sizeof(float), "x0_hist"}};
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
    auto extract = [&](float* cond, int, int v0, int n) { return launched(tile_extract_launch(noisy, cond, tg, v0, n, s), "tile_extract"); };
    if (int rc = run_passes(plan, extract, tiles, (int64_t)B * K, 1, th, tw, chw, L, member_rounds(sn), sc, flags, ws, stream)) return rc;
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
    if (int rc = apply_dpm(clip_x0, x0_hist, &sc)) return rc;
    if (n_iters > 0 && !x0_hist) return fail(MI_EINVAL, "null argument");
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

// ---------------------------------------------------------------------------- tiled denoising, the tiles fused after every step
extern "C" int mi_tile_consensus(float* tiles, int B, int C, int H, int W, int th, int tw, int oy, int ox, float* image_out, void* stream) {
    TileGeom g{};
    if (int rc = check_tile_run(B, C, H, W, th, tw, oy, ox, &g)) return rc;
    if (!tiles) return fail(MI_EINVAL, "null argument");
    const Buf buf[2] = {{tiles, (size_t)B * g.ny * g.nx * C * th * tw * sizeof(float), "tiles"},
                        {image_out, (size_t)B * C * H * W * sizeof(float), "image_out"}};
    if (int rc = check_no_overlap(buf, 2, "every pixel's value is written to its tile elements and to image_out in one launch")) return rc;
    return launched(tile_consensus_launch(tiles, image_out, B, g, (hipStream_t)stream), "tile_consensus");
}

// mi_denoise_tiled_fused behind its rule (include/midd.h: the composition it equals).  The steps are the OUTER loop: step i runs
// every pass as ONE ROW of the per-slot path -- the row mi_denoise_slots_rule would run for the pass: enqueue_run with the pass's
// slot tables -- and one consensus launch over all the tile states follows.  The condition tiles of every pass stay in the
// workspace for the whole call (tiled_fused_layout); x, the tile states, is tiles_out or the workspace.  As tiled_run: every rule
// is judged before the first launch, plan->side_mu is held over the call, the status word is cleared once and accumulates over
// all (step, pass) runs, every run joins its side streams (enqueue_run), no device memory is allocated and the host never waits.
static int tiled_fused_run(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out, float* x0_hist,
                           int B, int H, int W, int th, int tw, int oy, int ox, const Schedule& sc,
                           int seeded, uint64_t seed, int64_t sample_offset, int pass_samples, int flags,
                           void* workspace, size_t workspace_bytes, void* stream) {
    TileGeom tg{};
    if (int rc = check_tiled_args(plan, B, H, W, th, tw, oy, ox, sample_offset, pass_samples, &tg)) return rc;
    const int K = tg.ny * tg.nx;
    const int64_t V = (int64_t)B * K;
    const size_t chw = (size_t)tg.C * th * tw, img = (size_t)tg.C * H * W * sizeof(float), all = (size_t)V * chw * sizeof(float);
    const bool dpm = sc.rule == MI_UPDATE_DPMPP2M, ruled = sc.rule != MI_UPDATE_REFERENCE;
    const Buf buf[4] = {{noisy, (size_t)B * img, "noisy"}, {image_out, (size_t)B * img, "image_out"}, {tiles_out, all, "tiles_out"},
                        {dpm ? x0_hist : nullptr, all, "x0_hist"}};
    if (int rc = check_no_overlap(buf, 4, "noisy is read into the condition tiles, x0_hist beside the tiles by every step, and the consensus "
                                          "writes the tiles and image_out in one launch")) return rc;
    EnsembleLayout L{};
    // (evaluated before the state check, reported after it: check_batched_call; host arithmetic only, as in the *_workspace_bytes queries)
    const int layout_rc = tiled_fused_layout(plan, B, K, th, tw, pass_samples, tiles_out != nullptr, &L);
    if (int rc = check_batched_call(plan, layout_rc, L, workspace, workspace_bytes, {noisy, image_out}, sc)) return rc;
    Program *g_pass = nullptr, *g_tail = nullptr;            // the programs of a whole pass and of the shorter last one
    if (int rc = check_call(plan, L.pass, th, tw, workspace, L.run_bytes, &g_pass)) return rc;
    if (L.tail)
        if (int rc = check_call(plan, L.tail, th, tw, workspace, L.run_bytes, &g_tail)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* cond = reinterpret_cast<float*>(ws + L.cond_off);
    float* x = tiles_out ? tiles_out : reinterpret_cast<float*>(ws + L.samples_off);
    std::lock_guard<std::mutex> side_lk(plan->side_mu);     // held over all steps: the side streams are per plan
    HIPCHK(hipMemsetAsync(ws, 0, 256, s));                  // status word: once per call, the (step, pass) runs accumulate into it
    for (int64_t v0 = 0; v0 < V; v0 += 65535) {             // cond[v] = tile v of noisy; x[v] = cond[v]
        const int n = (int)(V - v0 < 65535 ? V - v0 : 65535);
        if (int rc = launched(tile_extract_launch(noisy, cond + (size_t)v0 * chw, tg, (int)v0, n, s), "tile_extract")) return rc;
    }
    HIPCHK(hipMemcpyAsync(x, cond, all, hipMemcpyDeviceToDevice, s));
    if (sc.n == 0) return launched(tile_blend_launch(x, image_out, B, tg, s), "tile_blend");      // no step: as mi_denoise_tiled
    // the slot tables of one row of one pass (host memory: enqueue_run reads them while it enqueues)
    std::vector<int32_t> t_row(L.pass), iter_base(L.pass), t_before(L.pass), t_after(L.pass);
    std::vector<int64_t> sample_index(L.pass);
    std::vector<uint32_t> frame((size_t)L.pass * 3);
    StepNoise sn;
    sn.seeded = seeded != 0; sn.seed = seed;
    for (int i = 0; i < sc.n; ++i) {
        for (int64_t v0 = 0; v0 < V; v0 += L.pass) {
            const int n = (int)(V - v0 < L.pass ? V - v0 : L.pass);
            for (int j = 0; j < n; ++j) {
                const int64_t v = v0 + j, b = v / K;
                const int k = (int)(v - b * K), ky = k / tg.nx, kx = k - ky * tg.nx;
                t_row[j] = sc.t[i]; iter_base[j] = i;
                t_before[j] = i > 0 ? sc.t[i - 1] : -1; t_after[j] = i + 1 < sc.n ? sc.t[i + 1] : -1;
                sample_index[j] = sample_offset + b;
                frame[(size_t)j * 3] = (uint32_t)W; frame[(size_t)j * 3 + 1] = (uint32_t)H * (uint32_t)W;
                frame[(size_t)j * 3 + 2] = (uint32_t)tile_origin(ky, H, th, tg.ny) * (uint32_t)W + (uint32_t)tile_origin(kx, W, tw, tg.nx);
            }
            Schedule row = sc;                               // the caller's tables and rule; one row, this pass's columns
            row.t = t_row.data(); row.n = 1; row.x0 = dpm ? x0_hist + (size_t)v0 * chw : nullptr; row.x0_stride = 0;
            const SlotRows slots{iter_base.data(), sample_index.data(), nullptr, seeded ? frame.data() : nullptr,
                                 ruled ? t_before.data() : nullptr, ruled ? t_after.data() : nullptr};
            if (int rc = enqueue_run(plan, n == L.pass ? g_pass : g_tail, cond + (size_t)v0 * chw, x + (size_t)v0 * chw, n, th, tw, row, &slots,
                                     sn, flags, ws, L.run_bytes, stream)) return rc;
        }
        if (int rc = launched(tile_consensus_launch(x, i == sc.n - 1 ? image_out : nullptr, B, tg, s), "tile_consensus")) return rc;
    }
    return MI_OK;
}

extern "C" int mi_denoise_tiled_fused(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out, float* x0_hist,
                                      int B, int H, int W, int th, int tw, int oy, int ox,
                                      const int32_t* t_list, int n_iters,
                                      const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                      int seeded, uint64_t seed, int64_t sample_offset, int pass_samples, int flags,
                                      const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream) {
    Schedule sc{t_list, n_iters, beta, alpha, alpha_hat, noise_steps};
    if (rule && rule->kind == MI_UPDATE_DPMPP2M) {
        if (seeded) return fail(MI_EINVAL, "seeded with MI_UPDATE_DPMPP2M: the rule is deterministic, it has no noise term (limit: seeded == 0)");
        if (int rc = apply_dpm(rule->clip_x0, x0_hist, &sc)) return rc;
        if (!x0_hist) return fail(MI_EINVAL, "MI_UPDATE_DPMPP2M without x0_hist: the rule reads every tile's previous predicted image (limit: x0_hist [B*tiles,C,th,tw] on the device)");
    } else {
        if (int rc = apply_rule(rule, &sc)) return rc;
        if (x0_hist) return fail(MI_EINVAL, "x0_hist with %s: the rule keeps no predicted image (limit: x0_hist NULL; MI_UPDATE_DPMPP2M takes it)",
                                 sc.rule == MI_UPDATE_DDIM ? "MI_UPDATE_DDIM" : "the reference's update");
    }
    return tiled_fused_run(plan, noisy, image_out, tiles_out, x0_hist, B, H, W, th, tw, oy, ox, sc, seeded, seed, sample_offset, pass_samples,
                           flags, workspace, workspace_bytes, stream);
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
    if (int rc = check_tile_run(B, C, H, W, th, tw, oy, ox, &g)) return rc;
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
    if (int rc = check_tile_run(B, C, H, W, th, tw, oy, ox, &g)) return rc;
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
    auto extract = [&](float* cond, int, int v0, int n) { return launched(tile_extract_launch(noisy, cond, tg, v0, n, s), "tile_extract"); };
    if (int rc = run_passes(plan, extract, tiles, (int64_t)B * K, members, th, tw, chw, L, member_rounds(sn), sc, flags, ws, stream)) return rc;      // V: ONE member's
    if (mean_out || std_out || samples_out)
        return launched(tile_blend_reduce_launch(tiles, B, members, tg, mean_out, std_out, samples_out, s), "tile_blend_reduce");
    return MI_OK;
}

// ---------------------------------------------------------------------------- geometric self-ensemble: flip / rotate views
// the view list of a call, host int32 -> the kernel argument (include/midd.h: THE GEOMETRY)
static int check_view_list(const int32_t* views, int n_views, DihedralViews* dv) {
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
    return MI_OK;
}

// ... and, where every view has the image's shape (the untiled calls), the rule of the transposing codes
static int check_views(const int32_t* views, int n_views, int H, int W, DihedralViews* dv) {
    if (int rc = check_view_list(views, n_views, dv)) return rc;
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
    auto fill = [&](float* cond, int, int v0, int n) { return launched(dihedral_views_launch(noisy, cond, dv, Cc, H, W, v0, n, s), "dihedral_views"); };
    if (int rc = run_passes(plan, fill, views_out, (int64_t)B * n_views, 1, H, W, chw, L, member_rounds(sn), sc, flags, ws, stream)) return rc;
    return launched(dihedral_reduce_launch(views_out, B, dv, Cc, H, W, mean_out, std_out, samples_out, s), "dihedral_reduce");
}

// ---------------------------------------------------------------------------- tiled self-ensemble: flip / rotate views at native size
// A transposed image is still cut into th x tw tiles, so H == W is not needed here; what a transposing code needs is that the
// W x H frame has as many tiles of the same shape (include/midd.h: THE GEOMETRY, "a view's tiles are the tiles of the viewed image")
static int check_view_tiles(const DihedralViews& dv, int th, int tw, int oy, int ox) {
    for (int k = 0; k < dv.n; ++k)
        if ((dv.code[k] & 4) && (th != tw || oy != ox))
            return fail(MI_EINVAL, "views[%d] = %d transposes the image, whose tiles are %dx%d with overlap %dx%d: the storage [views][B][tiles] holds "
                        "one tile count and shape for every view (limit: view codes 4 .. 7 need th == tw and oy == ox; H == W is not needed)",
                        k, (int)dv.code[k], th, tw, oy, ox);
    return MI_OK;
}

// the geometry of view `code`'s frame: the tiling of the viewed Hv x Wv image (tile_geometry.h)
static TileGeom view_frame(const TileGeom& g, int code) {
    return (code & 4) ? TileGeom{g.C, g.W, g.H, g.tw, g.th, g.ox, g.oy, g.nx, g.ny} : g;
}

// what the two stand-alone calls share: the geometry, the view list, the transposing rule, the batch and the tile blocks
static int check_unview_call(int B, int C, int H, int W, int th, int tw, int oy, int ox, const int32_t* views, int n_views, TileGeom* g, DihedralViews* dv) {
    if (int rc = check_tile_run(B, C, H, W, th, tw, oy, ox, g)) return rc;
    if (int rc = check_view_list(views, n_views, dv)) return rc;
    if (int rc = check_view_tiles(*dv, th, tw, oy, ox)) return rc;
    if (int rc = check_reduce_batch(B, "the limit of mi_ensemble_reduce, whose arithmetic this call composes")) return rc;
    return check_tiled_ensemble_size(B, n_views, *g);
}

extern "C" int mi_tile_blend_unview_reduce(const float* tiles, int B, int C, int H, int W, int th, int tw, int oy, int ox,
                                           const int32_t* views, int n_views, float* mean_out, float* std_out, float* samples_out, void* stream) {
    TileGeom g{};
    DihedralViews dv;
    if (int rc = check_unview_call(B, C, H, W, th, tw, oy, ox, views, n_views, &g, &dv)) return rc;
    if (!mean_out && !std_out && !samples_out) return fail(MI_EINVAL, "no output: give at least one of mean_out, std_out, samples_out");
    if (int rc = check_std_views(std_out, n_views)) return rc;
    if (!tiles) return fail(MI_EINVAL, "null argument");
    return launched(tile_blend_unview_reduce_launch(tiles, B, dv, g, mean_out, std_out, samples_out, (hipStream_t)stream), "tile_blend_unview_reduce");
}

extern "C" int mi_tile_blend_unview_quantiles(const float* tiles, int B, int C, int H, int W, int th, int tw, int oy, int ox,
                                              const int32_t* views, int n_views, const double* q, int nq, float* out, void* stream) {
    TileGeom g{};
    DihedralViews dv;
    if (int rc = check_unview_call(B, C, H, W, th, tw, oy, ox, views, n_views, &g, &dv)) return rc;
    QuantileLevels ql;
    if (int rc = check_quantile_levels(q, nq, &ql)) return rc;
    if (!tiles || !out) return fail(MI_EINVAL, "null argument");
    return launched(tile_blend_unview_quantiles_launch(tiles, B, dv, g, ql, out, (hipStream_t)stream), "tile_blend_unview_quantiles");
}

// the argument rules of mi_denoise_tiled_self_ensemble and of its workspace query, in the documented order (no GPU work)
static int check_tiled_self_ensemble_args(mi_plan* plan, int B, int H, int W, int th, int tw, int oy, int ox, const int32_t* views, int n_views,
                                          int64_t sample_offset, int64_t member_offset, int pass_samples, TileGeom* g, DihedralViews* dv) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (int rc = check_view_list(views, n_views, dv)) return rc;
    if (int rc = check_view_tiles(*dv, th, tw, oy, ox)) return rc;
    if (int rc = check_tiled_ensemble_args(plan, B, n_views, H, W, th, tw, oy, ox, sample_offset, member_offset, pass_samples, g)) return rc;
    return check_reduce_batch(B, "limit of the view and reduce kernels' grids");
}

// (the layout depends on the NUMBER of views alone; the list's transposing rule is judged by the call)
extern "C" size_t mi_tiled_self_ensemble_workspace_bytes(mi_plan* plan, int B, int n_views, int H, int W, int th, int tw, int oy, int ox,
                                                         int pass_samples, int tiles_external) {
    if (!plan) { fail(MI_EINVAL, "null plan"); return 0; }
    if (n_views < 1 || n_views > DIHEDRAL_MAX_VIEWS) {
        fail(MI_EINVAL, "n_views %d outside [1, %d]: a view list holds 1 to 8 distinct view codes (limit: 1 <= n_views <= %d)", n_views,
             DIHEDRAL_MAX_VIEWS, DIHEDRAL_MAX_VIEWS);
        return 0;
    }
    TileGeom g{};
    if (check_tiled_ensemble_args(plan, B, n_views, H, W, th, tw, oy, ox, 0, 0, pass_samples, &g)) return 0;
    if (check_reduce_batch(B, "limit of the view and reduce kernels' grids")) return 0;
    EnsembleLayout L{};
    size_t view_off = 0;
    if (tiled_self_ensemble_layout(plan, B, n_views, g.ny * g.nx, H, W, th, tw, pass_samples, tiles_external != 0, &L, &view_off)) return 0;
    return L.bytes;
}

// Views are the outer loop: round k is mi_denoise_tiled's pass structure over the viewed batch view(noisy, g_k) -- a copy in the
// workspace (plane_view_launch; the identity is read in place), cut by the extract of the view frame's geometry -- with the member
// word member_offset + k and that frame as the whole image of the seeded noise.  Its tiles are slice k of the storage
// [views][B][tiles], in the VIEW's frame; the final launch blends every view there, turns it back and reduces.
extern "C" int mi_denoise_tiled_self_ensemble(mi_plan* plan, const float* noisy, float* mean_out, float* std_out, float* samples_out, float* tiles_out,
                                              int B, int H, int W, int th, int tw, int oy, int ox, const int32_t* views, int n_views,
                                              const int32_t* t_list, int n_iters,
                                              const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                              int seeded, uint64_t seed, int64_t sample_offset, int64_t member_offset, int pass_samples, int flags,
                                              const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream) {
    Schedule sc{t_list, n_iters, beta, alpha, alpha_hat, noise_steps};
    if (rule && rule->kind == MI_UPDATE_DPMPP2M)
        return fail(MI_EINVAL, "update rule MI_UPDATE_DPMPP2M is not built for mi_denoise_tiled_self_ensemble: the call takes no buffer for the "
                    "predicted images (limit: MI_UPDATE_REFERENCE or MI_UPDATE_DDIM)");
    if (int rc = apply_rule(rule, &sc)) return rc;
    TileGeom tg{};
    DihedralViews dv;
    if (int rc = check_tiled_self_ensemble_args(plan, B, H, W, th, tw, oy, ox, views, n_views, sample_offset, member_offset, pass_samples, &tg, &dv))
        return rc;
    if (!mean_out && !std_out && !samples_out && !tiles_out)
        return fail(MI_EINVAL, "no output: give at least one of mean_out, std_out, samples_out, tiles_out");
    if (int rc = check_std_views(std_out, n_views)) return rc;
    const int K = tg.ny * tg.nx;
    const size_t chw = (size_t)tg.C * th * tw, img = (size_t)tg.C * H * W * sizeof(float);
    const Buf buf[5] = {{noisy, (size_t)B * img, "noisy"}, {mean_out, (size_t)B * img, "mean_out"}, {std_out, (size_t)B * img, "std_out"},
                        {samples_out, (size_t)B * n_views * img, "samples_out"},
                        {tiles_out, (size_t)n_views * B * K * chw * sizeof(float), "tiles_out"}};
    if (int rc = check_no_overlap(buf, 5, "noisy is read by every round and the reduce reads the tiles while it writes mean_out, std_out and samples_out"))
        return rc;
    EnsembleLayout L{};
    size_t view_off = 0;
    // (evaluated before the state check, reported after it: check_batched_call; host arithmetic only, as in the *_workspace_bytes queries)
    const int layout_rc = tiled_self_ensemble_layout(plan, B, n_views, K, H, W, th, tw, pass_samples, tiles_out != nullptr, &L, &view_off);
    if (int rc = check_batched_call(plan, layout_rc, L, workspace, workspace_bytes, {noisy}, sc)) return rc;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    float* tiles = tiles_out ? tiles_out : reinterpret_cast<float*>(ws + L.samples_off);
    float* viewed = reinterpret_cast<float*>(ws + view_off);
    std::lock_guard<std::mutex> side_lk(plan->side_mu);     // held over all passes: the side streams are per plan
    HIPCHK(hipMemsetAsync(ws, 0, 256, s));                  // status word: once per call, the passes of every view accumulate into it
    // round k draws as member member_offset + k, at the pixel's place in the whole VIEWED image (its frame: Hv x Wv, ny_v x nx_v tiles)
    auto noise = [&](int k) {
        StepNoise sn;
        if (seeded) {
            const TileGeom f = view_frame(tg, dv.code[k]);
            sn.seeded = true; sn.seed = seed; sn.sample_offset = sample_offset; sn.members = K; sn.member_offset = (uint32_t)(member_offset + k);
            sn.tiles_x = f.nx; sn.tiles_y = f.ny; sn.img_H = f.H; sn.img_W = f.W;
        }
        return sn;
    };
    // the first pass of a round makes the round's viewed copy (same stream: the passes of the round before have been enqueued and
    // joined), every pass extracts its tiles from it -- bit for bit the slices of view(noisy, g_k)
    auto fill = [&](float* cond, int k, int v0, int n) {
        const int code = dv.code[k];
        if (code != 0 && v0 == 0)
            if (int rc = launched(plane_view_launch(noisy, viewed, code, B, tg.C, H, W, s), "plane_view")) return rc;
        return launched(tile_extract_launch(code ? viewed : noisy, cond, view_frame(tg, code), v0, n, s), "tile_extract");
    };
    if (int rc = run_passes(plan, fill, tiles, (int64_t)B * K, n_views, th, tw, chw, L, noise, sc, flags, ws, stream)) return rc;      // V: ONE view's
    if (mean_out || std_out || samples_out)
        return launched(tile_blend_unview_reduce_launch(tiles, B, dv, tg, mean_out, std_out, samples_out, s), "tile_blend_unview_reduce");
    return MI_OK;
}
