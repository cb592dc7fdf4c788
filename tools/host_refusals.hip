// Host-side sanitizer harness for the executor, sampler, batched and analysis units (midd_exec.hip, midd_sampler.hip, midd_batched.hip,
// midd_analysis.hip): a stand-alone program that drives every mi_* entry of the four down a refusal path -- on an unfinalized plan
// where there is one -- with null, negative, overflowing, misaligned and aliasing arguments, and the two coefficient tables on 1-, 2-
// and 9-entry lists.  Nothing reaches a GPU: every call must return before its first launch, so it runs on a machine without one.
// Build the seven host units with the sanitizers on the host side only and link them with the kernel units of an ordinary build
// (make -C .../csrc):
//   C=medical-image-denoising-using-diffusion_amd/csrc; S="-Xarch_host -fsanitize=address,undefined -Xarch_host -fno-omit-frame-pointer"
//   U="midd_abi midd_weights midd_planner midd_exec midd_sampler midd_batched midd_analysis"
//   for u in $U; do hipcc -O1 -g -std=c++17 -fPIC --offload-arch=gfx950 $S -c $C/$u.hip -o /tmp/san_$u.o; done
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 $S -c tools/host_refusals.hip -o /tmp/san_main.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/san_*.o \
//     $(ls $C/build/*.o | grep -v $(printf -- "-e %s.o " $U)) -o /tmp/host_refusals
//   /tmp/host_refusals        # prints the number of calls checked; exit status 1 on a call that did not answer as expected
#include "../include/midd.h"
#include <cstdio>
#include <cstring>

static int bad = 0, n_calls = 0;
static void expect(bool refused, int rc, const char* what) {
    ++n_calls;
    if ((rc != MI_OK) != refused) { ++bad; printf("UNEXPECTED rc %d (%s): %s\n", rc, mi_last_error(), what); }
}
#define REFUSED(call) expect(true, (call), #call)
#define ACCEPTED(call) expect(false, (call), #call)

int main() {
    mi_unet_cfg cfg{};
    cfg.in_channels = 1; cfg.model_channels = 16; cfg.num_levels = 4;
    const int mult[4] = {1, 2, 3, 4};
    for (int i = 0; i < 4; ++i) cfg.channel_mult[i] = mult[i];
    cfg.num_res_blocks = 2; cfg.num_attention_levels = 1; cfg.attention_levels[0] = 3;
    cfg.time_emb_dim = 64; cfg.variant = MI_VARIANT_CDDPM; cfg.compute_mode = MI_COMPUTE_F16X3;
    mi_plan* p = nullptr;
    ACCEPTED(mi_unet_plan_create(&cfg, &p));
    if (!p) return 1;
    // "device pointers" that a refused call never reads, 1 MiB apart; WS is 256-byte aligned
    float *A = (float*)0x100000, *B_ = (float*)0x200000, *C_ = (float*)0x300000, *D = (float*)0x400000, *E = (float*)0x500000;
    void* WS = (void*)0x600000;
    const size_t WSB = 1 << 20;
    float tab[50];
    for (int i = 0; i < 50; ++i) tab[i] = 1e-4f + (0.02f - 1e-4f) * i / 49;
    float ah[50];
    double prod = 1.0;
    for (int i = 0; i < 50; ++i) { prod *= 1.0 - tab[i]; ah[i] = (float)prod; }
    const int32_t t3[3] = {40, 20, 0}, t_bad[3] = {40, 50, 0}, t_up[3] = {20, 40, 0};
    const int32_t t9[9] = {48, 42, 36, 30, 24, 18, 12, 6, 0};
    const mi_update_rule ddim{MI_UPDATE_DDIM, 0.5, 1}, eta_bad{MI_UPDATE_DDIM, 1.5, 1}, dpm{MI_UPDATE_DPMPP2M, 0.0, 1}, unknown{7, 0.0, 1};

    // ---- the coefficient tables: 1-, 2- and 9-entry lists, then their refusals
    float out[9 * 8];
    const int lens[3] = {1, 2, 9};
    for (int n : lens) {
        ACCEPTED(mi_ddim_coefficients(t9 + 9 - n, n, ah, 50, 0.5, out));
        ACCEPTED(mi_dpm_coefficients(t9 + 9 - n, n, ah, 50, out));
    }
    ACCEPTED(mi_ddim_coefficients(nullptr, 0, ah, 50, 0.0, nullptr));
    REFUSED(mi_ddim_coefficients(t3, 3, ah, 50, -0.1, out));
    REFUSED(mi_ddim_coefficients(t3, -1, ah, 50, 0.0, out));
    REFUSED(mi_ddim_coefficients(nullptr, 3, ah, 50, 0.0, out));
    REFUSED(mi_ddim_coefficients(t3, 3, nullptr, 50, 0.0, out));
    REFUSED(mi_ddim_coefficients(t3, 3, ah, 0, 0.0, out));
    REFUSED(mi_ddim_coefficients(t_bad, 3, ah, 50, 0.0, out));
    REFUSED(mi_ddim_coefficients(t_up, 3, ah, 50, 0.0, out));
    REFUSED(mi_ddim_coefficients(t3, 3, tab, 50, 0.0, out));      // an increasing table: alpha_hat[t_i] > alpha_hat[t_{i+1}]
    REFUSED(mi_ddim_coefficients(t3, 3, ah, 50, 0.0, nullptr));
    REFUSED(mi_dpm_coefficients(t_up, 3, ah, 50, out));
    REFUSED(mi_dpm_coefficients(t3, 3, ah, 50, nullptr));

    // ---- midd_exec.hip
    REFUSED(mi_unet_forward(nullptr, A, B_, t3, C_, 2, 32, 32, WS, WSB, nullptr));
    REFUSED(mi_unet_forward(p, A, B_, t3, C_, 2, 32, 32, WS, WSB, nullptr));
    REFUSED(mi_debug_fetch(nullptr, "out_conv", 2, 32, 32, WS, A, nullptr, nullptr, nullptr, nullptr));
    REFUSED(mi_debug_fetch(p, nullptr, 2, 32, 32, WS, A, nullptr, nullptr, nullptr, nullptr));
    REFUSED(mi_debug_fetch(p, "out_conv", 2, 32, 32, WS, A, nullptr, nullptr, nullptr, nullptr));
    REFUSED(mi_profile_begin(nullptr));
    int n_entries = -1;
    REFUSED(mi_profile_end(nullptr, nullptr, 0, &n_entries));
    REFUSED(mi_profile_end(p, nullptr, 0, nullptr));
    ACCEPTED(mi_profile_begin(p));
    ACCEPTED(mi_profile_end(p, nullptr, 0, &n_entries));      // no spans: no event is touched

    // ---- midd_sampler.hip
    REFUSED(mi_denoise(nullptr, A, B_, 2, 32, 32, t3, 3, tab, tab, ah, 50, nullptr, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise(p, A, A, 2, 32, 32, t3, -1, nullptr, tab, ah, 2000, nullptr, 0, nullptr, 0, nullptr));
    REFUSED(mi_denoise_seeded(nullptr, A, B_, 2, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_seeded(p, A, B_, 2, 32, 32, t3, 3, tab, tab, ah, 50, 5, -2, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_seeded(p, A, B_, 2, 0, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_seeded(p, A, B_, 2, 65536, 65536, t3, 3, tab, tab, ah, 50, 5, 0, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_seeded(p, A, B_, 2, 32, 32, t_bad, 3, tab, tab, ah, 50, 5, 0, 0, (char*)WS + 4, WSB, nullptr));
    REFUSED(mi_denoise_rule(p, A, B_, 2, 32, 32, t3, 3, tab, tab, ah, 50, nullptr, 0, 0, 0, 0, &eta_bad, WS, WSB, nullptr));
    REFUSED(mi_denoise_rule(p, A, B_, 2, 32, 32, t3, 3, tab, tab, ah, 50, nullptr, 0, 0, 0, 0, &dpm, WS, WSB, nullptr));
    REFUSED(mi_denoise_rule(p, A, B_, 2, 32, 32, t3, 3, tab, tab, ah, 50, nullptr, 0, 0, 0, 0, &unknown, WS, WSB, nullptr));
    REFUSED(mi_denoise_rule(p, A, B_, 2, 32, 32, t_up, 3, tab, tab, ah, 50, nullptr, 0, 0, 0, 0, &ddim, WS, WSB, nullptr));
    REFUSED(mi_denoise_rule(p, A, B_, 2, 32, 32, t3, 3, tab, tab, ah, 50, C_, 1, 5, 0, 0, &ddim, WS, WSB, nullptr));
    REFUSED(mi_denoise_rule(nullptr, A, B_, 2, 32, 32, t3, 3, tab, tab, ah, 50, nullptr, 1, 5, 0, 0, &ddim, WS, WSB, nullptr));
    REFUSED(mi_denoise_rule(p, A, B_, 2, 32, 32, t3, 3, tab, tab, ah, 50, nullptr, 1, 5, -1, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_rule(p, A, B_, 2, 32, 32, t3, 3, tab, tab, ah, 50, nullptr, 0, 0, 0, 0, &ddim, WS, WSB, nullptr));
    REFUSED(mi_denoise_dpm(p, A, B_, C_, 1, 2, 32, 32, t_up, 3, tab, tab, ah, 50, 0, 1, WS, WSB, nullptr));
    REFUSED(mi_denoise_dpm(p, A, B_, C_, 2, 2, 32, 32, t3, 3, tab, tab, ah, 50, 0, 1, WS, WSB, nullptr));
    REFUSED(mi_denoise_dpm(nullptr, A, B_, C_, 1, 2, 32, 32, t3, 3, tab, tab, ah, 50, 0, 1, WS, WSB, nullptr));
    REFUSED(mi_denoise_dpm(p, A, B_, nullptr, 1, 2, 32, 32, t3, 3, tab, tab, ah, 50, 0, 1, WS, WSB, nullptr));
    REFUSED(mi_denoise_dpm(p, A, B_, C_, 1, 0, 32, 32, t3, 3, tab, tab, ah, 50, 0, 1, WS, WSB, nullptr));
    REFUSED(mi_denoise_dpm(p, A, B_, A + 8, 3, 2, 32, 32, t3, 3, tab, tab, ah, 50, 0, 1, WS, WSB, nullptr));
    REFUSED(mi_denoise_dpm(p, A, B_, C_, 3, 2, 32, 32, t3, 3, tab, tab, ah, 50, 0, 1, WS, WSB, nullptr));
    const int32_t rows[6] = {40, 40, 20, 20, 0, 0}, rows_back[6] = {40, -1, 20, 20, 0, 0}, rows_bad[6] = {40, 50, 20, 20, 0, 0};
    const int32_t ib_bad[2] = {-1, 0}, ib_top[2] = {2147483647, 0};
    const int64_t si_bad[2] = {0, -4};
    REFUSED(mi_denoise_slots(nullptr, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, nullptr, B_, 2, 32, 32, rows, 3, nullptr, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 2, 32, 32, rows, -1, nullptr, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 0, 32, 32, rows, 3, nullptr, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, tab, tab, ah, 0, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 2, 32, 32, rows_bad, 3, nullptr, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 2, 32, 32, rows_back, 3, nullptr, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 2, 32, 32, rows, 3, ib_bad, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 2, 32, 32, rows, 3, ib_top, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 2, 32, 32, rows, 3, nullptr, si_bad, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, tab, tab, ah, 50, C_, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 2, 65536, 65536, rows, 3, nullptr, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, A + 4, 2, 32, 32, rows, 3, nullptr, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    // the virtual-sample tables: member words and (pitch, plane, origin) frames, the 64-bit sum at the top of the uint32 range included
    const int64_t mb_ok[2] = {3, ((int64_t)1 << 32) - 1}, mb_neg[2] = {0, -1}, mb_top[2] = {(int64_t)1 << 32, 0};
    const uint32_t fr_ok[6] = {88, 88 * 104, 0, 88, 88 * 104, 72 * 88 + 56}, fr_pitch[6] = {32, 1024, 0, 31, 1024, 0};
    const uint32_t fr_origin[6] = {32, 1024, 0, 40, 1280, 9}, fr_wrap[6] = {0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 32, 1024, 0};
    REFUSED(mi_denoise_slots_virtual(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, mb_neg, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots_virtual(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, mb_top, nullptr, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots_virtual(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, nullptr, fr_pitch, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots_virtual(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, nullptr, fr_origin, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots_virtual(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, nullptr, fr_wrap, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots_virtual(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, mb_ok, nullptr, tab, tab, ah, 50, nullptr, 0, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots_virtual(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, nullptr, fr_ok, tab, tab, ah, 50, C_, 0, 5, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_slots_virtual(p, A, B_, 2, 32, 32, rows, 3, nullptr, nullptr, mb_ok, fr_ok, tab, tab, ah, 50, nullptr, 1, 5, 0, WS, WSB, nullptr));      // valid: the state check
    REFUSED(mi_step_noise_fill(A, 2, 2, 1, 32, 32, 5, -1, nullptr));
    REFUSED(mi_step_noise_fill(A, 2, 2, 1, 65536, 65536, 5, 0, nullptr));
    REFUSED(mi_step_noise_fill(A, 65536, 2, 1, 32, 32, 5, 0, nullptr));
    REFUSED(mi_step_noise_fill(nullptr, 2, 2, 1, 32, 32, 5, 0, nullptr));
    REFUSED(mi_step_noise_fill_member(A, 2, 2, 1, 32, 32, 5, 0, -1, nullptr));
    REFUSED(mi_step_noise_fill_member(A, 2, 2, 1, 32, 32, 5, 0, (int64_t)1 << 32, nullptr));
    ACCEPTED(mi_step_noise_fill_member(nullptr, 0, 2, 1, 32, 32, 5, 0, 0, nullptr));

    // ---- midd_analysis.hip: the stand-alone reduce, quantile, scores, modes and spectrum calls
    const double q_ok[2] = {0.1, 0.9}, q_bad[2] = {0.1, 1.5};
    REFUSED(mi_ensemble_reduce(A, 2, 0, 1024, B_, C_, nullptr));
    REFUSED(mi_ensemble_reduce(A, 65536, 4, 1024, B_, C_, nullptr));
    REFUSED(mi_ensemble_reduce(A, 2, 4, (int64_t)1 << 32, B_, C_, nullptr));
    REFUSED(mi_ensemble_reduce(A, 2, 1, 1024, B_, C_, nullptr));
    REFUSED(mi_ensemble_reduce(nullptr, 2, 4, 1024, B_, C_, nullptr));
    REFUSED(mi_ensemble_quantiles(A, 2, 0, 1024, q_ok, 2, B_, nullptr));
    REFUSED(mi_ensemble_quantiles(A, 0, 4, 1024, q_ok, 2, B_, nullptr));
    REFUSED(mi_ensemble_quantiles(A, 2, 4, 0, q_ok, 2, B_, nullptr));
    REFUSED(mi_ensemble_quantiles(A, 2, 1 << 20, 1024, q_ok, 2, B_, nullptr));
    REFUSED(mi_ensemble_quantiles(A, 2, 4, 1024, q_ok, 0, B_, nullptr));
    REFUSED(mi_ensemble_quantiles(A, 2, 4, 1024, nullptr, 2, B_, nullptr));
    REFUSED(mi_ensemble_quantiles(A, 2, 4, 1024, q_bad, 2, B_, nullptr));
    REFUSED(mi_ensemble_quantiles(A, 2, 4, 1024, q_ok, 2, nullptr, nullptr));
    // (8-byte aligned outputs at 1 MiB steps: doubles F, G; the unsigned counters U1 .. U3 of the scores and modes; the signed counts
    // I1 .. I3 of the spectra)
    double *F = (double*)0x700000, *G = (double*)0x800000;
    uint64_t *U1 = (uint64_t*)0x900000, *U2 = (uint64_t*)0xA00000, *U3 = (uint64_t*)0xB00000;
    int64_t *I1 = (int64_t*)0xC00000, *I2 = (int64_t*)0xD00000, *I3 = (int64_t*)0xE00000;
    REFUSED(mi_ensemble_scores_workspace_bytes(0, 4, 1024) == 0);
    REFUSED(mi_ensemble_scores_workspace_bytes(2, 65, 1024) == 0);
    ACCEPTED(mi_ensemble_scores_workspace_bytes(2, 4, 1024) == 0);
    REFUSED(mi_ensemble_scores(A, B_, 0, 4, 1024, q_ok, 2, F, U1, U2, U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 65, 1024, q_ok, 2, F, U1, U2, U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 4, (int64_t)1 << 32, q_ok, 2, F, U1, U2, U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 4, 1024, q_ok, 9, F, U1, U2, U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 4, 1024, q_bad, 2, F, U1, U2, U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 4, 1024, nullptr, 2, F, U1, U2, U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 4, 1024, q_ok, 2, nullptr, U1, U2, U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 4, 1024, q_ok, 2, F, U1, U2, nullptr, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 4, 1024, nullptr, 0, F, U1, U2, U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 4, 1024, q_ok, 2, F, (uint64_t*)((char*)U1 + 4), U2, U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, (float*)((char*)B_ + 2), 2, 4, 1024, q_ok, 2, F, U1, U2, U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 4, 1024, q_ok, 2, F, U1, U2, U3, C_, WS, 8, nullptr));
    REFUSED(mi_ensemble_scores(A, B_, 2, 4, 1024, q_ok, 2, F, U1, (uint64_t*)(F + 1), U3, C_, WS, WSB, nullptr));
    REFUSED(mi_ensemble_gram_workspace_bytes(2, 1, 1024) == 0);
    ACCEPTED(mi_ensemble_gram_workspace_bytes(2, 12, 5000) == 0);
    REFUSED(mi_ensemble_gram(A, 65536, 4, 1024, F, U1, WS, WSB, nullptr));
    REFUSED(mi_ensemble_gram(A, 2, 1, 1024, F, U1, WS, WSB, nullptr));
    REFUSED(mi_ensemble_gram(A, 2, 4, 0, F, U1, WS, WSB, nullptr));
    REFUSED(mi_ensemble_gram(A, 2, 4, 1024, nullptr, U1, WS, WSB, nullptr));
    REFUSED(mi_ensemble_gram(A, 2, 4, 1024, (double*)((char*)F + 4), U1, WS, WSB, nullptr));
    REFUSED(mi_ensemble_gram((float*)((char*)A + 1), 2, 4, 1024, F, U1, WS, WSB, nullptr));
    REFUSED(mi_ensemble_gram(A, 2, 4, 1024, F, U1, WS, 8, nullptr));
    REFUSED(mi_ensemble_gram(A, 2, 4, 1024, F, (uint64_t*)(F + 2), WS, WSB, nullptr));
    REFUSED(mi_ensemble_project(A, 2, 65, 1024, F, 2, B_, nullptr));
    REFUSED(mi_ensemble_project(A, 2, 4, 1024, F, 9, B_, nullptr));
    REFUSED(mi_ensemble_project(A, 2, 4, 1024, nullptr, 2, B_, nullptr));
    REFUSED(mi_ensemble_project(A, 2, 4, 1024, (double*)((char*)F + 4), 2, B_, nullptr));
    REFUSED(mi_ensemble_project(A, 2, 4, 1024, F, 2, (float*)((char*)B_ + 2), nullptr));
    REFUSED(mi_ensemble_project(A, 2, 4, 1024, F, 2, A + 8, nullptr));
    // the spectra: the host window is the one thing a refusal path reads, and only after every other rule (32 entries, the last not finite)
    float win[32];
    for (int i = 0; i < 32; ++i) win[i] = 0.5f;
    win[31] = win[31] / 0.0f;
    const size_t nps_ws = mi_noise_power_spectrum_workspace_bytes(2, 3, 1, 70, 83, 32, 16), xs_ws = mi_cross_spectrum_workspace_bytes(2, 3, 3, 1, 70, 83, 32, 16);
    ACCEPTED(nps_ws == 0 || xs_ws == 0);
    REFUSED(mi_noise_power_spectrum_workspace_bytes(2, 3, 1, 70, 83, 48, 16) == 0);
    REFUSED(mi_noise_power_spectrum_workspace_bytes(1, 17, 1, 46371, 46371, 32, 1) == 0);
    REFUSED(mi_cross_spectrum_workspace_bytes(2, 2, 3, 1, 70, 83, 32, 16) == 0);
    REFUSED(mi_noise_power_spectrum(A, B_, 2, 3, 1, 70, 83, 48, 16, 2, win, 1.0, 0, F, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, B_, 2, 3, 1, 70, 83, 32, 0, 2, win, 1.0, 0, F, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, B_, 65536, 3, 1, 70, 83, 32, 16, 2, win, 1.0, 0, F, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, B_, 2, 3, 1, 31, 83, 32, 16, 2, win, 1.0, 0, F, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, B_, 2, 3, 1, 70000, 70000, 32, 1, 2, win, 1.0, 0, F, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, B_, 2, 3, 1, 70, 83, 32, 16, 3, win, 1.0, 0, F, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, B_, 2, 3, 1, 70, 83, 32, 16, 2, win, 1.0, 2, F, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, B_, 2, 3, 1, 70, 83, 32, 16, 2, win, 1.0 / 0.0, 0, F, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, nullptr, 2, 3, 1, 70, 83, 32, 16, 2, win, 1.0, 0, nullptr, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, B_, 2, 3, 1, 70, 83, 32, 16, 2, win, 1.0, 0, F, (double*)((char*)G + 4), I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, (float*)((char*)B_ + 1), 2, 3, 1, 70, 83, 32, 16, 2, win, 1.0, 0, F, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, B_, 2, 3, 1, 70, 83, 32, 16, 2, win, 1.0, 0, F, G, I1, I2, I3, WS, nps_ws - 1, nullptr));
    REFUSED(mi_noise_power_spectrum(A, A + 70 * 83, 2, 3, 1, 70, 83, 32, 16, 2, win, 1.0, 0, F, G, I1, I2, I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, B_, 2, 3, 1, 70, 83, 32, 16, 2, win, 1.0, 0, F, G, I1, (int64_t*)(F + 1), I3, WS, nps_ws, nullptr));
    REFUSED(mi_noise_power_spectrum(A, nullptr, 2, 3, 1, 70, 83, 32, 16, 2, win, 1.0, 0, F, G, I1, I2, I3, WS, nps_ws, nullptr));      // valid but for the window
    REFUSED(mi_cross_spectrum(A, B_, 2, 3, 0, 1, 70, 83, 32, 16, 2, win, 0, F, G, I1, I2, I3, WS, xs_ws, nullptr));
    REFUSED(mi_cross_spectrum(A, B_, 2, 2, 3, 1, 70, 83, 32, 16, 2, win, 0, F, G, I1, I2, I3, WS, xs_ws, nullptr));
    REFUSED(mi_cross_spectrum(A, B_, 2, 3, 3, 1, 70, 83, 64, 16, 2, win, 0, F, G, I1, I2, I3, WS, xs_ws, nullptr));      // (roi 64: a valid shape, the workspace of roi 32)
    REFUSED(mi_cross_spectrum(A, B_, 2, 3, 3, 1, 70, 83, 32, 16, -1, win, 0, F, G, I1, I2, I3, WS, xs_ws, nullptr));
    REFUSED(mi_cross_spectrum(A, B_, 2, 3, 3, 1, 70, 83, 32, 16, 2, win, -1, F, G, I1, I2, I3, WS, xs_ws, nullptr));
    REFUSED(mi_cross_spectrum(A, nullptr, 2, 3, 3, 1, 70, 83, 32, 16, 2, win, 0, F, G, I1, I2, I3, WS, xs_ws, nullptr));
    REFUSED(mi_cross_spectrum(A, B_, 2, 3, 3, 1, 70, 83, 32, 16, 2, win, 0, F, G, I1, I2, (int64_t*)((char*)I3 + 2), WS, xs_ws, nullptr));
    REFUSED(mi_cross_spectrum((float*)((char*)A + 2), B_, 2, 3, 3, 1, 70, 83, 32, 16, 2, win, 0, F, G, I1, I2, I3, WS, xs_ws, nullptr));
    REFUSED(mi_cross_spectrum(A, B_, 2, 3, 3, 1, 70, 83, 32, 16, 2, win, 0, F, G, I1, I2, I3, WS, 0, nullptr));
    REFUSED(mi_cross_spectrum(A, B_, 2, 3, 3, 1, 70, 83, 32, 16, 2, win, 0, (double*)(B_ + 2), G, I1, I2, I3, WS, xs_ws, nullptr));
    REFUSED(mi_cross_spectrum(A, B_, 2, 3, 3, 1, 70, 83, 32, 16, 2, win, 0, F, F + 4 * 2 * 32 * 32 - 1, I1, I2, I3, WS, xs_ws, nullptr));
    REFUSED(mi_cross_spectrum(A, A, 2, 3, 3, 1, 70, 83, 32, 16, 2, win, 0, F, G, I1, I2, I3, WS, xs_ws, nullptr));      // x == y is allowed: the window
    // ---- midd_batched.hip: the stand-alone tile and view calls
    int n_tiles = 0, origins[8];
    ACCEPTED(mi_tile_geometry(90, 32, 8, &n_tiles, origins, 8));
    ACCEPTED(mi_tile_geometry(90, 32, 8, &n_tiles, origins, 1));      // more tiles than `cap`: only cap origins are written
    REFUSED(mi_tile_geometry(90, 0, 8, &n_tiles, origins, 8));
    REFUSED(mi_tile_geometry(16, 32, 8, &n_tiles, origins, 8));
    REFUSED(mi_tile_geometry(90, 32, 17, &n_tiles, origins, 8));
    REFUSED(mi_tile_geometry(90, 32, 8, nullptr, origins, 8));
    REFUSED(mi_tile_extract(A, 2, 0, 90, 70, 32, 32, 8, 8, 0, 4, B_, nullptr));
    REFUSED(mi_tile_extract(A, 2, 1, 90, 70, 96, 32, 8, 8, 0, 4, B_, nullptr));
    REFUSED(mi_tile_extract(A, 2, 1, 92680, 70, 92680, 32, 46340, 8, 0, 4, B_, nullptr));
    REFUSED(mi_tile_extract(A, 0, 1, 90, 70, 32, 32, 8, 8, 0, 4, B_, nullptr));
    REFUSED(mi_tile_extract(A, 1 << 30, 1, 64, 64, 32, 32, 0, 0, 0, 4, B_, nullptr));
    REFUSED(mi_tile_extract(A, 2, 1, 90, 70, 32, 32, 8, 8, 2147483647, 4, B_, nullptr));
    REFUSED(mi_tile_extract(A, 2, 4, 65536, 65536, 32768, 32768, 0, 0, 0, 4, B_, nullptr));
    REFUSED(mi_tile_extract(nullptr, 2, 1, 90, 70, 32, 32, 8, 8, 0, 4, B_, nullptr));
    REFUSED(mi_tile_blend(A, 2, 0, 90, 70, 32, 32, 8, 8, B_, nullptr));
    REFUSED(mi_tile_blend(A, 2, 1, 90, 70, 32, 72, 8, 8, B_, nullptr));
    REFUSED(mi_tile_blend(A, 0, 1, 90, 70, 32, 32, 8, 8, B_, nullptr));
    REFUSED(mi_tile_blend(A, 1, 1, 65536, 65536, 32, 32, 8, 8, B_, nullptr));
    REFUSED(mi_tile_blend(A, 2, 1, 90, 70, 32, 32, 8, 8, nullptr, nullptr));
    REFUSED(mi_tile_blend_reduce(A, 2, 3, 0, 90, 70, 32, 32, 8, 8, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_reduce(A, 2, 3, 1, 90, 70, 32, 32, -1, 8, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_reduce(A, 1, 3, 1, 65536, 65536, 32, 32, 8, 8, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_reduce(A, 2, 0, 1, 90, 70, 32, 32, 8, 8, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_reduce(A, 65536, 3, 1, 64, 64, 32, 32, 0, 0, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_reduce(A, 1 << 15, 1 << 15, 1, 64, 64, 32, 32, 0, 0, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_reduce(A, 2, 1, 1, 90, 70, 32, 32, 8, 8, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_reduce(A, 2, 3, 1, 90, 70, 32, 32, 8, 8, nullptr, C_, D, nullptr));
    REFUSED(mi_tile_blend_quantiles(A, 2, 3, 0, 90, 70, 32, 32, 8, 8, q_ok, 2, B_, nullptr));
    REFUSED(mi_tile_blend_quantiles(A, 2, 3, 1, 90, 70, 32, 32, 8, 17, q_ok, 2, B_, nullptr));
    REFUSED(mi_tile_blend_quantiles(A, 1, 3, 1, 65536, 65536, 32, 32, 8, 8, q_ok, 2, B_, nullptr));
    REFUSED(mi_tile_blend_quantiles(A, 2, 0, 1, 90, 70, 32, 32, 8, 8, q_ok, 2, B_, nullptr));
    REFUSED(mi_tile_blend_quantiles(A, 2, 1 << 20, 1, 90, 70, 32, 32, 8, 8, q_ok, 2, B_, nullptr));
    REFUSED(mi_tile_blend_quantiles(A, 2, 3, 1, 90, 70, 32, 32, 8, 8, q_bad, 2, B_, nullptr));
    REFUSED(mi_tile_blend_quantiles(A, 2, 3, 1, 90, 70, 32, 32, 8, 8, q_ok, 2, nullptr, nullptr));
    const int32_t v_ok[2] = {0, 3}, v_rep[2] = {3, 3}, v_code[2] = {0, 8}, v_t[2] = {0, 5};
    REFUSED(mi_dihedral_views(A, 2, 0, 32, 32, v_ok, 2, 0, 4, B_, nullptr));
    REFUSED(mi_dihedral_views(A, 2, 1, 65536, 65536, v_ok, 2, 0, 4, B_, nullptr));
    REFUSED(mi_dihedral_views(A, 2, 1, 32, 32, v_ok, 9, 0, 4, B_, nullptr));
    REFUSED(mi_dihedral_views(A, 2, 1, 32, 32, nullptr, 2, 0, 4, B_, nullptr));
    REFUSED(mi_dihedral_views(A, 2, 1, 32, 32, v_rep, 2, 0, 4, B_, nullptr));
    REFUSED(mi_dihedral_views(A, 2, 1, 32, 32, v_code, 2, 0, 4, B_, nullptr));
    REFUSED(mi_dihedral_views(A, 2, 1, 32, 40, v_t, 2, 0, 4, B_, nullptr));
    REFUSED(mi_dihedral_views(A, 0, 1, 32, 32, v_ok, 2, 0, 4, B_, nullptr));
    REFUSED(mi_dihedral_views(A, 2, 1, 32, 32, v_ok, 2, 2147483647, 4, B_, nullptr));
    REFUSED(mi_dihedral_views(nullptr, 2, 1, 32, 32, v_ok, 2, 0, 4, B_, nullptr));
    REFUSED(mi_dihedral_reduce(A, 2, 1, 32, 32, v_ok, 0, B_, C_, D, nullptr));
    REFUSED(mi_dihedral_reduce(A, 2, 1, 32, 32, v_ok, 2, nullptr, nullptr, nullptr, nullptr));
    REFUSED(mi_dihedral_reduce(A, 2, 1, 32, 32, v_ok, 1, B_, C_, D, nullptr));
    REFUSED(mi_dihedral_reduce(nullptr, 2, 1, 32, 32, v_ok, 2, B_, C_, D, nullptr));
    REFUSED(mi_dihedral_quantiles(A, 2, 1, 32, 32, v_rep, 2, q_ok, 2, B_, nullptr));
    REFUSED(mi_dihedral_quantiles(A, 2, 1, 32, 32, v_ok, 2, q_bad, 2, B_, nullptr));
    REFUSED(mi_dihedral_quantiles(A, 2, 1, 32, 32, v_ok, 2, q_ok, 2, nullptr, nullptr));

    const int32_t v_d4[8] = {0, 1, 2, 3, 4, 5, 6, 7};
    REFUSED(mi_tile_blend_unview_reduce(A, 2, 0, 90, 70, 32, 32, 8, 8, v_ok, 2, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(A, 2, 1, 90, 70, 32, 32, 17, 8, v_ok, 2, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(A, 2, 1, 90, 70, 32, 32, 8, 8, v_ok, 0, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(A, 2, 1, 90, 70, 32, 32, 8, 8, nullptr, 2, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(A, 2, 1, 90, 70, 32, 32, 8, 8, v_rep, 2, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(A, 2, 1, 90, 70, 32, 32, 8, 8, v_code, 2, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(A, 2, 1, 90, 70, 32, 64, 8, 8, v_t, 2, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(A, 2, 1, 90, 70, 32, 32, 8, 4, v_d4, 8, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(A, 65536, 1, 64, 64, 32, 32, 0, 0, v_ok, 2, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(A, 2, 1, 90, 70, 32, 32, 8, 8, v_d4, 8, nullptr, nullptr, nullptr, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(A, 2, 1, 90, 70, 32, 32, 8, 8, v_t + 1, 1, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_reduce(nullptr, 2, 1, 90, 70, 32, 32, 8, 8, v_d4, 8, B_, C_, D, nullptr));
    REFUSED(mi_tile_blend_unview_quantiles(A, 2, 1, 90, 70, 32, 64, 8, 8, v_t, 2, q_ok, 2, B_, nullptr));
    REFUSED(mi_tile_blend_unview_quantiles(A, 2, 1, 90, 70, 32, 32, 8, 8, v_d4, 8, q_bad, 2, B_, nullptr));
    REFUSED(mi_tile_blend_unview_quantiles(A, 2, 1, 90, 70, 32, 32, 8, 8, v_d4, 8, q_ok, 9, B_, nullptr));
    REFUSED(mi_tile_blend_unview_quantiles(A, 2, 1, 90, 70, 32, 32, 8, 8, v_d4, 8, q_ok, 2, nullptr, nullptr));

    // ---- midd_batched.hip: the four batched calls and their rule / dpm forms
    REFUSED(mi_denoise_ensemble(nullptr, A, B_, C_, nullptr, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble(p, A, B_, C_, nullptr, 2, 0, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble(p, A, B_, C_, nullptr, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, -1, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble(p, A, B_, C_, nullptr, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, ((int64_t)1 << 32) - 3, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble(p, A, B_, C_, nullptr, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 0, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble(p, A, B_, C_, nullptr, 65535, 1 << 20, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble(p, A, B_, C_, nullptr, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, -2, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble(p, A, nullptr, nullptr, nullptr, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble(p, A, B_, C_, nullptr, 2, 1, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble(p, A, B_, B_ + 8, nullptr, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble(p, A, B_, C_, D, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble_rule(p, A, B_, C_, D, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, &eta_bad, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble_rule(p, A, B_, C_, D, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, &dpm, WS, WSB, nullptr));
    REFUSED(mi_denoise_ensemble_rule(p, A, B_, C_, D, 2, 4, 32, 32, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, &ddim, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled(nullptr, A, B_, nullptr, 2, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled(p, A, B_, nullptr, 2, 90, 70, 36, 32, 8, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled(p, A, B_, nullptr, 2, 90, 70, 32, 32, 17, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled(p, A, B_, nullptr, 2, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled(p, A, B_, nullptr, 2, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 1, 5, -2, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled(p, A, B_, nullptr, 1 << 30, 64, 64, 32, 32, 0, 0, t3, 3, tab, tab, ah, 50, 1, 5, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled(p, A, A + 8, nullptr, 2, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled(p, A, B_, C_, 2, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_rule(p, A, B_, C_, 2, 90, 70, 32, 32, 8, 8, t_up, 3, tab, tab, ah, 50, 1, 5, 0, 16, 0, &ddim, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_rule(p, A, B_, C_, 2, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 16, 0, &ddim, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_dpm(p, A, B_, C_, D, 2, 90, 70, 32, 32, 8, 8, t_up, 3, tab, tab, ah, 50, 16, 0, 1, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_dpm(p, A, B_, C_, nullptr, 2, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 16, 0, 1, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_dpm(p, A, B_, C_, A + 8, 2, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 16, 0, 1, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_dpm(p, A, B_, C_, D, 2, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 16, 0, 1, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_ensemble(nullptr, A, B_, C_, nullptr, nullptr, 2, 3, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 0, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_ensemble(p, A, B_, C_, nullptr, nullptr, 1 << 20, 1 << 10, 64, 64, 32, 32, 0, 0, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_ensemble(p, A, nullptr, nullptr, nullptr, nullptr, 2, 3, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 1, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_ensemble(p, A, B_, C_, D, D + 8, 2, 3, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_ensemble(p, A, B_, C_, D, E, 2, 3, 90, 70, 32, 32, 8, 8, t3, 3, tab, tab, ah, 50, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_self_ensemble(nullptr, A, B_, C_, nullptr, 2, 32, 32, v_ok, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_self_ensemble(p, A, B_, C_, nullptr, 2, 32, 32, v_rep, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_self_ensemble(p, A, B_, C_, nullptr, 2, 32, 40, v_t, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_self_ensemble(p, A, B_, C_, nullptr, 2, 32, 32, v_ok, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, -1, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_self_ensemble(p, A, nullptr, nullptr, nullptr, 2, 32, 32, v_ok, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_self_ensemble(p, A, B_, C_, nullptr, 2, 32, 32, v_ok, 1, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_self_ensemble(p, A, A + 8, C_, nullptr, 2, 32, 32, v_ok, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    REFUSED(mi_denoise_self_ensemble(p, A, B_, C_, D, 2, 32, 32, v_ok, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, WS, WSB, nullptr));
    // the tiled self-ensemble: the rule, the view list, the transposing rule, then the tiled ensemble's rules with members = n_views
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, &dpm, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, &eta_bad, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_d4, 8, t_up, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, &ddim, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(nullptr, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_d4, 9, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, nullptr, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_rep, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_code, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 64, 8, 8, v_t, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 4, v_t, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 36, 36, 8, 8, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, -2, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, ((int64_t)1 << 32) - 7, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 0, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 1 << 28, 64, 64, 32, 32, 0, 0, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 65536, 64, 64, 32, 32, 0, 0, v_ok, 2, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, nullptr, nullptr, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, nullptr, nullptr, 2, 90, 70, 32, 32, 8, 8, v_t + 1, 1, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, D, D + 8, 2, 90, 70, 32, 32, 8, 8, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, nullptr, WS, WSB, nullptr));
    REFUSED(mi_denoise_tiled_self_ensemble(p, A, B_, C_, D, E, 2, 41, 27, 16, 16, 4, 4, v_d4, 8, t3, 3, tab, tab, ah, 50, 1, 5, 0, 0, 16, 0, &ddim, WS, WSB, nullptr));      // valid, all 8 views of a non-square image: the state check

    mi_plan_destroy(p);
    printf("%d calls, %d unexpected\n", n_calls, bad);
    return bad ? 1 : 0;
}
