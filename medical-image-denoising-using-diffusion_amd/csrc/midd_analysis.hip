// The stand-alone analysis calls (no plan, no schedule, no pass): the reduce and quantile maps of an ensemble, its scores against a
// truth, its principal modes, the channel responses of a model observer, the noise power spectrum and the cross-spectrum.  Each judges its rules in the order include/midd.h
// documents, before anything is read, and ends in one launch wrapper.  The member / batch / level rules that the batched calls
// (midd_batched.hip) compose are defined here and declared in midd_sampler.h.
#include <algorithm>
#include <cstdio>
#include "midd_sampler.h"

using namespace midd;

// ---------------------------------------------------------------------------- the rules stated once
int midd::check_members_min(int members) {
    return members >= 1 ? MI_OK : fail(MI_EINVAL, "members %d: an ensemble has at least one member (limit: members >= 1)", members);
}

int midd::check_std_members(const float* std_out, int members) {
    if (std_out && members < 2) return fail(MI_EINVAL, "std_out needs members >= 2: the unbiased standard deviation of one value is undefined");
    return MI_OK;
}

// B is grid.y of the reduce kernel
int midd::check_reduce_batch(int B, const char* why) {
    return (B >= 1 && B <= 65535) ? MI_OK : fail(MI_EINVAL, "B %d outside [1, 65535] (%s)", B, why);
}

// the members of a pixel are sorted in registers (ensemble.hip: ensemble_quantiles_kernel): at most QUANTILE_MAX_MEMBERS of them
int midd::check_quantile_members(int members) {
    if (members > QUANTILE_MAX_MEMBERS)
        return fail(MI_EINVAL, "members %d: the quantile kernels sort a pixel's members in registers (limit: members <= %d; mean and std have no such limit)",
                    members, QUANTILE_MAX_MEMBERS);
    return MI_OK;
}

// the levels of a call, host doubles -> the kernel argument.  nq_min: 1 for the quantile calls, 0 for the scores (no coverage counts)
int midd::check_quantile_levels(const double* q, int nq, QuantileLevels* ql, int nq_min) {
    if (nq < nq_min || nq > QUANTILE_MAX_LEVELS)
        return fail(MI_EINVAL, "nq %d outside [%d, %d]: the levels travel as kernel arguments (limit: %d <= nq <= %d)", nq, nq_min, QUANTILE_MAX_LEVELS,
                    nq_min, QUANTILE_MAX_LEVELS);
    if (nq > 0 && !q) return fail(MI_EINVAL, "null argument");
    *ql = QuantileLevels{};
    ql->nq = nq;
    for (int i = 0; i < nq; ++i) {
        if (!(q[i] >= 0.0 && q[i] <= 1.0)) return fail(MI_EINVAL, "q[%d] = %.17g outside [0, 1] (limit: 0 <= q <= 1, not NaN)", i, q[i]);
        ql->q[i] = q[i];
    }
    return MI_OK;
}

// the elements of a sample
static int check_chw(int64_t chw) {
    if (chw < 1 || chw >= MEMBER_WORDS) return fail(MI_EINVAL, "chw %lld outside [1, 2^32) (limit: C*H*W < 4294967296)", (long long)chw);
    return MI_OK;
}

// every pointer of the list on a multiple of `align` bytes (a null one is); `text` is the call's whole sentence
static int check_aligned(std::initializer_list<const void*> ptrs, uintptr_t align, const char* text) {
    for (const void* p : ptrs)
        if (reinterpret_cast<uintptr_t>(p) & (align - 1)) return fail(MI_EINVAL, "%s", text);
    return MI_OK;
}

// `query` names the call that answers `need`
static int check_workspace_size(size_t got, size_t need, const char* query) {
    return got >= need ? MI_OK : fail(MI_EINVAL, "workspace too small: need %zu bytes (%s), got %zu", need, query, got);
}

static_assert(sizeof(long long) == sizeof(int64_t), "the counters are 64-bit");
static unsigned long long* counters(uint64_t* p) { return reinterpret_cast<unsigned long long*>(p); }
static long long* counters(int64_t* p) { return reinterpret_cast<long long*>(p); }

// ---------------------------------------------------------------------------- mean, std and quantile maps
// what the two calls open with: the members, the batch, the elements of a sample
static int check_ensemble_run(int B, int members, int64_t chw) {
    if (int rc = check_members_min(members)) return rc;
    if (int rc = check_reduce_batch(B)) return rc;
    return check_chw(chw);
}

extern "C" int mi_ensemble_reduce(const float* samples, int B, int members, int64_t chw, float* mean_out, float* std_out, void* stream) {
    if (int rc = check_ensemble_run(B, members, chw)) return rc;
    if (int rc = check_std_members(std_out, members)) return rc;
    if (!samples || !mean_out) return fail(MI_EINVAL, "null argument");
    return launched(ensemble_reduce_launch(samples, B, members, (unsigned long long)chw, mean_out, std_out, (hipStream_t)stream), "ensemble_reduce");
}

extern "C" int mi_ensemble_quantiles(const float* samples, int B, int members, int64_t chw, const double* q, int nq, float* out, void* stream) {
    if (int rc = check_ensemble_run(B, members, chw)) return rc;
    if (int rc = check_quantile_members(members)) return rc;
    QuantileLevels ql;
    if (int rc = check_quantile_levels(q, nq, &ql)) return rc;
    if (!samples || !out) return fail(MI_EINVAL, "null argument");
    return launched(ensemble_quantiles_launch(samples, B, members, (unsigned long long)chw, ql, out, (hipStream_t)stream), "ensemble_quantiles");
}

// ---------------------------------------------------------------------------- the scores against a truth image
// (ensemble_scores.hip; include/midd.h: THE ENSEMBLE SCORES)
static int check_scores_shape(int B, int members, int64_t chw) {
    if (int rc = check_reduce_batch(B, "limit of the scores kernel's grid")) return rc;
    if (members < 1 || members > QUANTILE_MAX_MEMBERS)
        return fail(MI_EINVAL, "members %d outside [1, %d]: the scores kernel sorts a pixel's members in registers (limit: 1 <= members <= %d)",
                    members, QUANTILE_MAX_MEMBERS, QUANTILE_MAX_MEMBERS);
    return check_chw(chw);
}

extern "C" size_t mi_ensemble_scores_workspace_bytes(int B, int members, int64_t chw) {
    if (check_scores_shape(B, members, chw)) return 0;
    return ensemble_scores_partials_bytes(B, (unsigned long long)chw);
}

extern "C" int mi_ensemble_scores(const float* samples, const float* truth, int B, int members, int64_t chw, const double* q, int nq,
                                  double* sums, uint64_t* invalid, uint64_t* rank_hist, uint64_t* counts, float* crps_map,
                                  void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_scores_shape(B, members, chw)) return rc;
    QuantileLevels ql;
    if (int rc = check_quantile_levels(q, nq, &ql, 0)) return rc;
    if (!samples || !truth || !sums || !invalid || !rank_hist || !workspace) return fail(MI_EINVAL, "null argument");
    if ((counts == nullptr) != (nq == 0))
        return fail(MI_EINVAL, "counts and nq = %d disagree: counts holds [B][nq][2] counters and is NULL if and only if nq == 0", nq);
    if (int rc = check_aligned({sums, invalid, rank_hist, counts, workspace}, 8, "sums, invalid, rank_hist, counts and workspace must be 8-byte aligned")) return rc;
    if (int rc = check_aligned({samples, truth, crps_map}, 4, "samples, truth and crps_map must be 4-byte aligned")) return rc;
    const size_t need = ensemble_scores_partials_bytes(B, (unsigned long long)chw);
    if (int rc = check_workspace_size(workspace_bytes, need, "mi_ensemble_scores_workspace_bytes")) return rc;
    const size_t img = (size_t)chw * sizeof(float);
    const Buf buf[8] = {{samples, (size_t)B * members * img, "samples"}, {truth, (size_t)B * img, "truth"},
                        {sums, (size_t)B * 4 * sizeof(double), "sums"}, {invalid, (size_t)B * sizeof(uint64_t), "invalid"},
                        {rank_hist, (size_t)B * (2 * members + 1) * sizeof(uint64_t), "rank_hist"},
                        {counts, (size_t)B * nq * 2 * sizeof(uint64_t), "counts"}, {crps_map, (size_t)B * img, "crps_map"},
                        {workspace, need, "workspace"}};
    if (int rc = check_no_overlap(buf, 8, "samples and truth are read while every output and the workspace are written")) return rc;
    return launched(ensemble_scores_launch(samples, truth, B, members, (unsigned long long)chw, ql, sums, counters(invalid), counters(rank_hist),
                                           counters(counts), crps_map, static_cast<double*>(workspace), (hipStream_t)stream), "ensemble_scores");
}

// ---------------------------------------------------------------------------- the principal modes of an ensemble's spread
// (ensemble_modes.hip; include/midd.h: THE ENSEMBLE MODES): the Gram matrix of the centred members and the projection onto the
// caller's weight rows
static int check_modes_shape(int B, int members, int64_t chw) {
    if (int rc = check_reduce_batch(B, "limit of the modes kernels' grid")) return rc;
    if (members < 2 || members > MODES_MAX_MEMBERS)
        return fail(MI_EINVAL, "members %d outside [2, %d]: one member has no spread, and the Gram kernel tiles at most %d members (limit: 2 <= members <= %d)",
                    members, MODES_MAX_MEMBERS, MODES_MAX_MEMBERS, MODES_MAX_MEMBERS);
    return check_chw(chw);
}

extern "C" size_t mi_ensemble_gram_workspace_bytes(int B, int members, int64_t chw) {
    if (check_modes_shape(B, members, chw)) return 0;
    return ensemble_gram_workspace_bytes(B, members, (unsigned long long)chw);
}

extern "C" int mi_ensemble_gram(const float* samples, int B, int members, int64_t chw, double* gram, uint64_t* invalid,
                                void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_modes_shape(B, members, chw)) return rc;
    if (!samples || !gram || !invalid || !workspace) return fail(MI_EINVAL, "null argument");
    if (int rc = check_aligned({gram, invalid, workspace}, 8, "gram, invalid and workspace must be 8-byte aligned")) return rc;
    if (int rc = check_aligned({samples}, 4, "samples must be 4-byte aligned")) return rc;
    const size_t need = ensemble_gram_workspace_bytes(B, members, (unsigned long long)chw);
    if (int rc = check_workspace_size(workspace_bytes, need, "mi_ensemble_gram_workspace_bytes")) return rc;
    const Buf buf[4] = {{samples, (size_t)B * members * (size_t)chw * sizeof(float), "samples"},
                        {gram, (size_t)B * members * members * sizeof(double), "gram"}, {invalid, (size_t)B * sizeof(uint64_t), "invalid"},
                        {workspace, need, "workspace"}};
    if (int rc = check_no_overlap(buf, 4, "samples is read while gram, invalid and the workspace are written")) return rc;
    return launched(ensemble_gram_launch(samples, B, members, (unsigned long long)chw, gram, counters(invalid), static_cast<double*>(workspace),
                                         (hipStream_t)stream), "ensemble_gram");
}

extern "C" int mi_ensemble_project(const float* samples, int B, int members, int64_t chw, const double* weights, int n_modes, float* out, void* stream) {
    if (int rc = check_modes_shape(B, members, chw)) return rc;
    if (n_modes < 1 || n_modes > MODES_MAX_MODES)
        return fail(MI_EINVAL, "n_modes %d outside [1, %d]: a projection launch holds at most %d accumulators per element (limit: 1 <= n_modes <= %d)",
                    n_modes, MODES_MAX_MODES, MODES_MAX_MODES, MODES_MAX_MODES);
    if (!samples || !weights || !out) return fail(MI_EINVAL, "null argument");
    if (int rc = check_aligned({weights}, 8, "weights must be 8-byte aligned")) return rc;
    if (int rc = check_aligned({samples, out}, 4, "samples and out must be 4-byte aligned")) return rc;
    const size_t img = (size_t)chw * sizeof(float);
    const Buf buf[3] = {{samples, (size_t)B * members * img, "samples"}, {weights, (size_t)B * n_modes * members * sizeof(double), "weights"},
                        {out, (size_t)B * n_modes * img, "out"}};
    if (int rc = check_no_overlap(buf, 3, "samples and weights are read while out is written")) return rc;
    return launched(ensemble_project_launch(samples, B, members, (unsigned long long)chw, weights, n_modes, out, (hipStream_t)stream), "ensemble_project");
}

// ---------------------------------------------------------------------------- the channel responses of a model observer
// (channel_responses.hip; include/midd.h: THE CHANNEL RESPONSES).  centres is a HOST table, as the timestep lists of the sampler calls
// are: its rule is judged here, before any GPU work
static int check_range(const char* name, int v, int lo, int hi, const char* why) {
    return (v >= lo && v <= hi) ? MI_OK : fail(MI_EINVAL, "%s %d outside [%d, %d] (%s)", name, v, lo, hi, why);
}

extern "C" int mi_channel_responses(const float* x, int N, int H, int W, const int32_t* centres, int L, int R, const double* channels, int C,
                                    double* out, uint32_t* invalid, void* stream) {
    if (int rc = check_range("N", N, 1, CR_MAX_PLANES, "limit of the kernel's grid")) return rc;
    if (int rc = check_range("H", H, 1, CR_MAX_SIDE, "an ROI origin travels as two 16-bit kernel arguments")) return rc;
    if (int rc = check_range("W", W, 1, CR_MAX_SIDE, "an ROI origin travels as two 16-bit kernel arguments")) return rc;
    if (int rc = check_range("R", R, CR_MIN_ROI, CR_MAX_ROI, "the side of an ROI, odd or even")) return rc;
    if (int rc = check_range("L", L, 1, CR_MAX_LOCATIONS, "the locations of a call")) return rc;
    if (int rc = check_range("C", C, 1, CR_MAX_CHANNELS, "the channels of a call")) return rc;
    if (!centres) return fail(MI_EINVAL, "null argument");                    // (the next rule reads it)
    for (int l = 0; l < L; ++l) {
        const int cy = centres[2 * l], cx = centres[2 * l + 1];
        const long long y0 = (long long)cy - R / 2, x0 = (long long)cx - R / 2;
        if (y0 < 0 || x0 < 0 || y0 + R > H || x0 + R > W)
            return fail(MI_EINVAL, "centre %d = (%d, %d): its ROI of side %d, rows %lld .. %lld and columns %lld .. %lld, leaves the %d x %d image "
                        "(an ROI is refused, not clipped)", l, cy, cx, R, y0, y0 + R - 1, x0, x0 + R - 1, H, W);
    }
    if (!x || !channels || !out || !invalid) return fail(MI_EINVAL, "null argument");
    if (int rc = check_aligned({channels, out}, 8, "channels and out must be 8-byte aligned")) return rc;
    if (int rc = check_aligned({x, invalid}, 4, "x and invalid must be 4-byte aligned")) return rc;
    const Buf buf[4] = {{x, (size_t)N * H * W * sizeof(float), "x"}, {channels, (size_t)C * R * R * sizeof(double), "channels"},
                        {out, (size_t)N * L * C * sizeof(double), "out"}, {invalid, (size_t)N * L * sizeof(uint32_t), "invalid"}};
    if (int rc = check_no_overlap(buf, 4, "x and channels are read while out and invalid are written")) return rc;
    return launched(channel_responses_launch(x, N, H, W, centres, L, R, channels, C, out, invalid, (hipStream_t)stream), "channel_responses");
}

// ---------------------------------------------------------------------------- the Welch spectra
// The noise power spectrum (nps.hip; include/midd.h: THE NOISE POWER SPECTRUM) and the cross-spectrum of two fields (cross_spectrum.hip;
// THE CROSS SPECTRUM).  The rules in the documented order; nothing is read, not even the host window, before every rule has passed
static int check_nps_shape(int B, int K, int C, int H, int W, int roi, int step) {
    if (roi != 32 && roi != 64 && roi != 128) return fail(MI_EINVAL, "roi %d outside {32, 64, 128}: the ROI transform is built for these sizes", roi);
    if (step < 1) return fail(MI_EINVAL, "step %d below 1 (limit: step >= 1)", step);
    if (B < 1 || K < 1 || C < 1) return fail(MI_EINVAL, "B %d, K %d, C %d: each must be at least 1", B, K, C);
    if ((long long)B * C > 65535) return fail(MI_EINVAL, "B * C = %lld groups outside [1, 65535] (limit of the kernel's grid)", (long long)B * C);
    if (H < roi || W < roi) return fail(MI_EINVAL, "image %d x %d smaller than the ROI %d x %d: there are no partial ROIs", H, W, roi, roi);
    const unsigned long long per_member = (unsigned long long)((H - roi) / step + 1) * (unsigned long long)((W - roi) / step + 1);
    if (per_member > 0x7FFFFFFFull || nps_chunks(K, H, W, roi, step) > 0x7FFFFFFFull)
        return fail(MI_EINVAL, "too many ROIs: %llu per member, K %d (limit: ROIs per member < 2^31, chunks of 16 ROIs < 2^31)", per_member, K);
    return MI_OK;
}

// the member rule, then the shape rules of the noise power spectrum with K = max(Kx, Ky)
static int check_xs_shape(int B, int Kx, int Ky, int C, int H, int W, int roi, int step) {
    if (Kx < 1 || Ky < 1) return fail(MI_EINVAL, "Kx %d, Ky %d: each field has at least one realisation", Kx, Ky);
    if (Kx != Ky && Kx != 1 && Ky != 1)
        return fail(MI_EINVAL, "Kx %d, Ky %d: the fields have K = max(Kx, Ky) members each, or one that is broadcast (limit: Kx, Ky in {K, 1})", Kx, Ky);
    return check_nps_shape(B, Kx > Ky ? Kx : Ky, C, H, W, roi, step);
}

extern "C" size_t mi_noise_power_spectrum_workspace_bytes(int B, int K, int C, int H, int W, int roi, int step) {
    if (check_nps_shape(B, K, C, H, W, roi, step)) return 0;
    return nps_workspace_bytes(B * C, K, H, W, roi, step);
}

extern "C" size_t mi_cross_spectrum_workspace_bytes(int B, int Kx, int Ky, int C, int H, int W, int roi, int step) {
    if (check_xs_shape(B, Kx, Ky, C, H, W, roi, step)) return 0;
    return xs_workspace_bytes(B * C, Kx > Ky ? Kx : Ky, H, W, roi, step);
}

// What follows the shape rules of a spectrum call, in the order in which it is reported: detrend, flags, the call's scale if it has
// one, the null pointers, the alignments, the workspace's size, the overlaps, the finite window.  in: the two fields, only read, the
// second one optional unless `both`; the cross-spectrum's may overlap each other, so each is judged against the outputs on its own
// (`both`), the NPS's may not (one table).  spectra: the call's first output; radial has a row of bins where it has a plane.  The
// sentences name the call's own buffers
struct SpectrumOut { double* radial; int64_t *radial_count, *rois_used, *rois_skipped; void* workspace; size_t workspace_bytes, need; const char* query; };

static int check_spectrum_call(int detrend, int flags, const double* scale, const Buf (&in)[2], bool both, const Buf& spectra, size_t groups, int roi,
                               const SpectrumOut& o, const float* window) {
    if (detrend < MI_NPS_DETREND_NONE || detrend > MI_NPS_DETREND_PLANE)
        return fail(MI_EINVAL, "detrend %d outside {0 none, 1 mean, 2 plane}", detrend);
    if (flags & ~MI_NPS_EXCLUDE_AXES) return fail(MI_EINVAL, "flags 0x%x: unknown bits (known: MI_NPS_EXCLUDE_AXES = 1)", (unsigned)flags);
    if (scale && (!(*scale == *scale) || *scale - *scale != 0.0)) return fail(MI_EINVAL, "scale %g is not finite", *scale);
    if (!in[0].p || (both && !in[1].p) || !spectra.p || !o.radial || !o.radial_count || !o.rois_used || !o.rois_skipped || !o.workspace)
        return fail(MI_EINVAL, "null argument");
    char text[128];
    snprintf(text, sizeof text, "%s, radial, radial_count, rois_used, rois_skipped and workspace must be 8-byte aligned", spectra.name);
    if (int rc = check_aligned({spectra.p, o.radial, o.radial_count, o.rois_used, o.rois_skipped, o.workspace}, 8, text)) return rc;
    snprintf(text, sizeof text, "%s and %s must be 4-byte aligned", in[0].name, in[1].name);
    if (int rc = check_aligned({in[0].p, in[1].p}, 4, text)) return rc;
    if (int rc = check_workspace_size(o.workspace_bytes, o.need, o.query)) return rc;
    const size_t bins = (size_t)roi / 2 + 1;
    snprintf(text, sizeof text, "%s and %s are read while every output and the workspace are written", in[0].name, in[1].name);
    const Buf all[8] = {in[0], in[1], spectra, {o.radial, spectra.bytes / ((size_t)roi * roi) * bins, "radial"},
                        {o.radial_count, bins * sizeof(int64_t), "radial_count"}, {o.rois_used, groups * sizeof(int64_t), "rois_used"},
                        {o.rois_skipped, groups * sizeof(int64_t), "rois_skipped"}, {o.workspace, o.need, "workspace"}};
    if (both) {                                   // in[0] and the outputs, then in[1] and the outputs
        Buf first[7] = {in[0]};
        std::copy(all + 2, all + 8, first + 1);
        if (int rc = check_no_overlap(first, 7, text)) return rc;
    }
    if (int rc = check_no_overlap(all + (both ? 1 : 0), both ? 7 : 8, text)) return rc;
    if (window)
        for (int i = 0; i < roi; ++i)
            if (!(window[i] == window[i]) || window[i] - window[i] != 0.0f) return fail(MI_EINVAL, "window[%d] is not finite", i);
    return MI_OK;
}

extern "C" int mi_noise_power_spectrum(const float* a, const float* b, int B, int K, int C, int H, int W, int roi, int step, int detrend,
                                       const float* window, double scale, int flags, double* nps, double* radial, int64_t* radial_count,
                                       int64_t* rois_used, int64_t* rois_skipped, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_nps_shape(B, K, C, H, W, roi, step)) return rc;
    const size_t groups = (size_t)B * C, img = (size_t)H * W * sizeof(float);
    const Buf in[2] = {{a, groups * K * img, "a"}, {b, groups * img, "b"}};
    const SpectrumOut out{radial, radial_count, rois_used, rois_skipped, workspace, workspace_bytes,
                          nps_workspace_bytes(B * C, K, H, W, roi, step), "mi_noise_power_spectrum_workspace_bytes"};
    if (int rc = check_spectrum_call(detrend, flags, &scale, in, false, {nps, groups * roi * roi * sizeof(double), "nps"}, groups, roi, out, window)) return rc;
    return launched(nps_launch(a, b, B, K, C, H, W, roi, step, detrend, window, scale, (flags & MI_NPS_EXCLUDE_AXES) ? 1 : 0, nps, radial,
                               counters(radial_count), counters(rois_used), counters(rois_skipped), workspace, (hipStream_t)stream), "noise_power_spectrum");
}

extern "C" int mi_cross_spectrum(const float* x, const float* y, int B, int Kx, int Ky, int C, int H, int W, int roi, int step, int detrend,
                                 const float* window, int flags, double* planes, double* radial, int64_t* radial_count,
                                 int64_t* rois_used, int64_t* rois_skipped, void* workspace, size_t workspace_bytes, void* stream) {
    if (int rc = check_xs_shape(B, Kx, Ky, C, H, W, roi, step)) return rc;
    const size_t groups = (size_t)B * C, img = (size_t)H * W * sizeof(float);
    const Buf in[2] = {{x, groups * Kx * img, "x"}, {y, groups * Ky * img, "y"}};
    const SpectrumOut out{radial, radial_count, rois_used, rois_skipped, workspace, workspace_bytes,
                          xs_workspace_bytes(B * C, Kx > Ky ? Kx : Ky, H, W, roi, step), "mi_cross_spectrum_workspace_bytes"};
    if (int rc = check_spectrum_call(detrend, flags, nullptr, in, true, {planes, 4 * groups * roi * roi * sizeof(double), "planes"}, groups, roi, out, window)) return rc;
    return launched(xs_launch(x, y, B, Kx, Ky, C, H, W, roi, step, detrend, window, (flags & MI_NPS_EXCLUDE_AXES) ? 1 : 0, planes, radial,
                              counters(radial_count), counters(rois_used), counters(rois_skipped), workspace, (hipStream_t)stream), "cross_spectrum");
}
