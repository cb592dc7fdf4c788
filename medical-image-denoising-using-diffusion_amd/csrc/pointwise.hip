// HBM-bound direct kernels at the two ends of the UNet and the resampling helpers.
//
//   in_conv_kernel   : Conv3x3(cat[x, condition]) 2*ic -> Cout        (DDIMModel.py:222-223)
//   out_conv_kernel  : GroupNorm-apply + SiLU + Conv3x3 C -> ic       (DDIMModel.py:213-217,248)
//                      fused with the sampler update of DiffusionDenoiser.denoise
//                      (DDIMModel.py:278-284; cddpm noise term cddpmModels.py:297-303)
//   out_conv_seeded_kernel : the same with the noise term drawn in the update (step_noise_common.h)
//   out_conv_ddim_kernel, out_conv_ddim_seeded_kernel : the same two with the DDIM(eta) update in the place of the reference's
//   out_conv_slots_kernel  : the same with every sample at its own timestep: coefficients, counter words and the active
//                      flag from the sample's SlotRec (mi_denoise_slots); slot_fill_kernel writes a row's records
//   step_noise_fill_kernel : the same noise values as a [n_iters,B,C,H,W] tensor (replay / export)
//   ensemble_reduce_kernel : mean and unbiased std over the members of an ensemble of stochastic samples
//   ensemble_broadcast_kernel : the condition image of an ensemble pass's virtual samples
//   tile_extract_kernel / tile_blend_kernel : overlapping network-sized tiles of a larger image, and their blend (mi_denoise_tiled)
//   tile_blend_reduce_kernel : blend of every member's tiles and mean / std over the blended members (mi_denoise_tiled_ensemble)
//   ensemble_quantiles_kernel / tile_blend_quantiles_kernel : per-pixel quantiles over the members, plain and blended from tiles
//   resize_bilinear  : F.interpolate(mode='bilinear', align_corners=False) (DDIMModel.py:242)
//   conv_transpose   : ConvTranspose2d(C,C,4,2,1) (DDIMModel.py:211) for topologies where the
//                      planner cannot fold it into a 3x3 (never on the default networks)
// K = 18 and N = 1 are degenerate GEMM shapes: these stay on the vector ALU and are judged
// against the HBM roofline.
#include "midd_internal.h"
#include "step_noise_common.h"
#include "tile_geometry.h"
#include "quantile_common.h"

namespace midd {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// x * sigmoid(x) on v_exp_f32 / v_rcp_f32 (~1 ulp each)
__device__ __forceinline__ float silu_pw(float v) {
    return v * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(v * -1.4426950408889634f));
}

// ------------------------------------------------------------------------------ statistics of a pointwise producer
// The two HBM-bound producers below also leave the GroupNorm totals of their output (stats_common.h) -- round 1/2 read the
// tensor a second time for that (chan_total_kernel: 4 launches per forward).  A workgroup owns a pixel range of ONE sample;
// thread = (pixel lane pl < ppi, channel group); each thread sums ITS NV channels over the pixels it walks (fp32, fixed
// order), the lanes are folded per channel in fp64 in lane order, rounded once to fp32, and published with exact integer
// atomics.  scratch: 2 * C * ppi floats of LDS; acc: (C + 2) * 6 words.
template <int NV>
__device__ __forceinline__ void pointwise_publish(const float (&sum)[NV], const float (&sq)[NV], bool active, int pl, int ppi, int cgrp,
                                                  int C, float* scratch, stat_word* acc, stat_word* tot, int b, int bs, int rep,
                                                  int replica, int tid, int nthreads = 256, int c0 = 0, int ncol = -1) {
    if (ncol < 0) ncol = C;                       // the workgroup's channels: [c0, c0 + ncol) of the tensor's C; cgrp counts inside them
    if (active) {
#pragma unroll
        for (int e = 0; e < NV; ++e) {
            scratch[(size_t)(cgrp * NV + e) * ppi + pl] = sum[e];
            scratch[(size_t)(ncol + cgrp * NV + e) * ppi + pl] = sq[e];
        }
    }
    auto fold = [&](int i) {
        double t = 0;
        for (int l = 0; l < ppi; ++l) t += (double)scratch[(size_t)i * ppi + l];
        return (float)t;
    };
    stat_publish(tot, b, C, bs, rep, replica, c0, ncol, fold, acc, tid, nthreads);
}

// pixels a workgroup of 256 threads walks: ~4 per pixel lane, at most 1024 workgroups per sample
static int pointwise_rows(int HW, int ppi) {
    int r = (HW + ppi * 4 - 1) / (ppi * 4);
    return r < 1 ? 1 : (r > 1024 ? 1024 : r);
}

// ------------------------------------------------------------------------------ in_conv
// thread = (pixel lane, 16 consecutive couts): the 18 input taps are loaded once per 16 outputs; weights
// [9][2ic][Cout] and bias staged in LDS; a pixel's lanes write one contiguous 4*Cout-byte run.  grid (rows, B).
__global__ __launch_bounds__(256)
void in_conv_kernel(const float* __restrict__ x, const float* __restrict__ cond, const float* __restrict__ w,
                    const float* __restrict__ bias, float* __restrict__ out, stat_word* __restrict__ tot, int rep, int bs,
                    int ic, int H, int W, int Cout, int rows, int blocked) {
    extern __shared__ float wl[];                 // 9*2ic*Cout + Cout, then the statistics scratch
    const int nw = 9 * 2 * ic * Cout;
    for (int i = threadIdx.x; i < nw + Cout; i += 256) wl[i] = (i < nw) ? w[i] : bias[i - nw];
    __syncthreads();
    const int CG = Cout >> 4;                     // groups of 16 couts
    const int ppi = 256 / CG;
    const int tid = threadIdx.x;
    const int pl = tid / CG, cg = tid - pl * CG;
    const bool active = pl < ppi;
    const int b = blockIdx.y, row = blockIdx.x;
    const int HW = H * W;
    const int per = (HW + rows - 1) / rows;
    const int p0 = row * per, p1 = min(HW, p0 + per);
    float ssum[16], ssq[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) { ssum[k] = 0.f; ssq[k] = 0.f; }
    if (active) {
        for (int p = p0 + pl; p < p1; p += ppi) {
            const int oy = p / W, ox = p - oy * W;
            f32x4 acc[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) acc[k] = *reinterpret_cast<const f32x4*>(&wl[nw + cg * 16 + k * 4]);
            for (int ci = 0; ci < 2 * ic; ++ci) {
                const float* plane = (ci < ic) ? x + ((size_t)b * ic + ci) * HW
                                               : cond + ((size_t)b * ic + (ci - ic)) * HW;
#pragma unroll
                for (int dy = 0; dy < 3; ++dy) {
                    const int gy = oy + dy - 1;
                    if (gy < 0 || gy >= H) continue;
#pragma unroll
                    for (int dx = 0; dx < 3; ++dx) {
                        const int gx = ox + dx - 1;
                        if (gx < 0 || gx >= W) continue;
#if defined(PW_ABL) && PW_ABL == 3      // ablation (tools/mb/pw_abl.hip, wrong results): no input loads
                        const float v = 1.0f + (float)gx;
#else
                        const float v = plane[(size_t)gy * W + gx];
#endif
                        const float* wr = &wl[((dy * 3 + dx) * 2 * ic + ci) * Cout + cg * 16];
#if defined(PW_ABL) && PW_ABL == 4      // ablation: no weight reads / multiply-adds
                        acc[dx] += v;
#else
#pragma unroll
                        for (int k = 0; k < 4; ++k) acc[k] += v * *reinterpret_cast<const f32x4*>(wr + k * 4);
#endif
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
#if defined(PW_ABL) && PW_ABL == 1      // ablation: no output stores
                if (acc[k][0] == 12345.678f)
#endif
                *reinterpret_cast<f32x4*>(out + act_index(blocked, b, Cout, HW, p, cg * 16 + k * 4)) = acc[k];
#if !(defined(PW_ABL) && PW_ABL == 2)   // ablation: no statistics
#pragma unroll
                for (int e = 0; e < 4; ++e) { ssum[k * 4 + e] += acc[k][e]; ssq[k * 4 + e] += acc[k][e] * acc[k][e]; }
#endif
            }
        }
    }
    if (tot == nullptr) return;
    float* const scratch = wl + nw + Cout;
    stat_word* const acc_lds = reinterpret_cast<stat_word*>(scratch + 2 * (size_t)Cout * ppi + (((nw + Cout) & 1) ? 1 : 0));   // 8-byte aligned
    pointwise_publish<16>(ssum, ssq, active, pl, ppi, cg, Cout, scratch, acc_lds, tot, b, bs, rep, row % rep, tid);
}


// ------------------------------------------------------------------------------ in_conv, one input channel (the reference's grayscale case)
// Round 3.  Ablations (tools/mb/pw_abl.hip) of the kernel above at B = 4: 36 us, 23 of them with the stores removed -- it
// is bound by its instruction stream and its latencies (72 per-lane LDS weight reads and a branch per tap for 288
// multiply-adds; three threads load each pixel's taps; 1.5 waves per SIMD), and its stores, 16 bytes per lane 64 bytes
// apart, reach 2.4 TB/s where contiguous ones reach 4 (tools/mb/hbm_rate.hip).  Here every WAVE works on its own:
//   lane = pixel, all Cout outputs of it: the weights are uniform -- broadcast reads from LDS, half of the couts at a time with
//   the next tap's quads requested before this tap's multiply-adds (as scalar loads with SGPR operands they
//   cost 620 cycles per tap: SMEM returns out of order, every use waits for all of it) -- the 18 taps are loaded once per
//   pixel, branch-free from clamped addresses, coalesced, one pass ahead;
//   the wave's [64 pixels][Cout] tile is turned through its OWN LDS patch (no workgroup barrier in the loop) and
//   leaves as whole contiguous rows, every lane 16 bytes next to its neighbour's;
//   the statistics are summed on the values in store order: a lane meets NQ / gcd(64, NQ) different channel quads.
// Same accumulation order per output as above: bias, then (channel, dy, dx).  grid (rows, B), 4 waves.
template <int COUT, bool BLOCKED>
__global__ __launch_bounds__(256, 3)
void in_conv1_kernel(const float* __restrict__ x, const float* __restrict__ cond, const float* __restrict__ w,
                     const float* __restrict__ bias, float* __restrict__ out, stat_word* __restrict__ tot, int rep, int bs,
                     int H, int W, int per) {
    constexpr int NQ = COUT / 4;                                  // 16-byte pieces per pixel
    constexpr int G64 = (NQ % 16 == 0) ? 16 : (NQ % 8 == 0) ? 8 : (NQ % 4 == 0) ? 4 : (NQ % 2 == 0) ? 2 : 1;   // gcd(64, NQ)
    // NHWC output: store order = pixel-major quads, a lane meets NQ / gcd(64, NQ) different quads; channel-blocked output
    // [B][COUT/16][HW][16] (BLOCKED, midd_internal.h): store order = block, pixel, quad -- a lane meets quad lane % 4 of every block
    constexpr int SETS = BLOCKED ? COUT / 16 : NQ / G64;          // channel quads a lane meets in store order
    constexpr int PS = COUT + 4;                                  // padded pixel stride (words): 16-byte stores of 8 lanes on distinct banks
    constexpr int SLOTS = BLOCKED ? 64 : 4 * SETS * ((64 + NQ - 1) / NQ);   // contributors per channel: (wave, lane / 4) | (wave, set, lane / NQ)
    extern __shared__ __attribute__((aligned(16))) float ic1_lds[];   // [4 waves][64][PS] tiles; afterwards the statistics scratch [2][COUT][SLOTS]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    float* const tile = ic1_lds + wave * (64 * PS);
    float* const wlds = ic1_lds + 4 * 64 * PS + ((COUT + 2) * STAT_WORDS * 2 + 4);      // behind the tiles and the publish accumulators: [18][COUT] weights, [COUT] bias
    for (int i = tid; i < 19 * COUT; i += 256) wlds[i] = (i < 18 * COUT) ? w[i] : bias[i - 18 * COUT];
    __syncthreads();
    const int b = blockIdx.y, HW = H * W;
    const int p0 = blockIdx.x * per, p1 = min(HW, p0 + per);
    const float* const xp = x + (size_t)b * HW;
    const float* const cp = cond + (size_t)b * HW;
    float ssum[SETS][4], ssq[SETS][4];
#pragma unroll
    for (int j = 0; j < SETS; ++j)
#pragma unroll
        for (int e = 0; e < 4; ++e) { ssum[j][e] = 0.f; ssq[j][e] = 0.f; }
    auto load_taps = [&](int base, float (&v)[18]) {
        const int pc = min(base + lane, HW - 1);
        const int oy = pc / W, ox = pc - oy * W;
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int gy = oy + dy - 1, cy = min(max(gy, 0), H - 1);
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int gx = ox + dx - 1, cx = min(max(gx, 0), W - 1);
                const bool in = (gy == cy) && (gx == cx);
#if defined(PW_ABL) && PW_ABL == 6      // ablation (tools/mb/pw_abl.hip, wrong results): no input loads
                const float a0 = (float)cx, a1 = (float)cy;
#else
                const float a0 = xp[cy * W + cx], a1 = cp[cy * W + cx];
#endif
                v[dy * 3 + dx] = in ? a0 : 0.f;
                v[9 + dy * 3 + dx] = in ? a1 : 0.f;
            }
        }
    };
    float vn[18];
    int base = p0 + wave * 64;
    if (base < p1) load_taps(base, vn);
    for (; base < p1; base += 256) {
        float v[18];
#pragma unroll
        for (int i = 0; i < 18; ++i) v[i] = vn[i];
        if (base + 256 < p1) load_taps(base + 256, vn);           // next pass's taps fly under this pass's arithmetic
        // Weights from LDS (uniform address: a broadcast read), half of the couts at a time so that the NEXT tap's quads fit in
        // registers beside the accumulators: LDS reads return in order, the compiler's counted waits keep several in flight.
        // (Scalar loads return out of order: every use waits for ALL of them, lgkmcnt(0) -- one tap in flight, ~620 cycles per tap.)
        int wofs = 0;                                             // opaque per pass: otherwise the weights are hoisted out of the pass loop
        asm volatile("" : "+v"(wofs));
        const float* const wl = wlds + wofs;
        constexpr int NQH = NQ / 2;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            f32x4 acc[NQH], wv[2][NQH];
            auto wload = [&](int i, f32x4 (&d)[NQH]) {
#pragma unroll
                for (int q = 0; q < NQH; ++q) d[q] = *reinterpret_cast<const f32x4*>(wl + ((i % 9) * 2 + i / 9) * COUT + (h * NQH + q) * 4);
            };
#pragma unroll
            for (int q = 0; q < NQH; ++q) acc[q] = *reinterpret_cast<const f32x4*>(wl + 18 * COUT + (h * NQH + q) * 4);
            wload(0, wv[0]);
#pragma unroll
            for (int i = 0; i < 18; ++i) {
                if (i + 1 < 18) wload(i + 1, wv[(i + 1) & 1]);
                // The multiply-adds are written out as v_pk_fma_f32 with the tap in the LOW dword of an aligned register pair and
                // `op_sel_hi:[1,0,1]` (both results read src1's low dword).  hipcc's own choice for a tap that sits in the HIGH dword
                // of a pair (the taps are consecutive registers: v[1] was the one) is `op_sel:[0,1,0]` -- the low result selects
                // src1's high dword -- and THAT form intermittently drops its low-half product (D.lo = C.lo) in lanes 48..63 when the
                // workgroup shares its CU with another kernel's waves: round 3's red split-sampler case (DESIGN.md section 2a;
                // A/B of nothing but the operand selection, 600 concurrent forwards each: 0 vs 367 corrupted, every tap hit).
                // tests/test_isa_audit_cpu.py fails the build if any shipped kernel carries a packed-fp32 op with an `op_sel:` bit set.
                {
                    typedef float f32x2 __attribute__((ext_vector_type(2)));
                    f32x2 tp = {v[i], v[i]};
#pragma unroll
                    for (int q = 0; q < NQH; ++q) {
                        f32x2 a0 = {acc[q][0], acc[q][1]}, a1 = {acc[q][2], acc[q][3]};
                        const f32x2 w0 = {wv[i & 1][q][0], wv[i & 1][q][1]}, w1 = {wv[i & 1][q][2], wv[i & 1][q][3]};
                        asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(a0) : "v"(w0), "v"(tp));
                        asm volatile("v_pk_fma_f32 %0, %1, %2, %0 op_sel_hi:[1,0,1]" : "+v"(a1) : "v"(w1), "v"(tp));
                        acc[q] = (f32x4){a0[0], a0[1], a1[0], a1[1]};
                    }
                }
#pragma unroll
                for (int q = 0; q < NQH; ++q) asm volatile("" : "+v"(acc[q]));      // pinned: not sunk to the tile stores with all weights live
            }
#pragma unroll
            for (int q = 0; q < NQH; ++q) *reinterpret_cast<f32x4*>(&tile[lane * PS + (h * NQH + q) * 4]) = acc[q];
        }
        // the wave's own patch: its LDS operations execute in order, no barrier
        const int npx = min(64, p1 - base);
#pragma unroll
        for (int r = 0; r < NQ; ++r) {
            int px, c, set; float* dst;
            if constexpr (BLOCKED) {                              // block r / 4: 64 pixels x 64 bytes, contiguous
                const int k = r >> 2, idx = (r & 3) * 64 + lane;
                px = idx >> 2; c = k * 4 + (idx & 3); set = k;
                dst = out + (((size_t)b * (COUT / 16) + k) * HW + base) * 16 + (size_t)idx * 4;
            } else {
                const int idx = r * 64 + lane;
                px = idx / NQ; c = idx - px * NQ; set = r % SETS;
                dst = out + ((size_t)b * HW + base) * COUT + (size_t)idx * 4;
            }
            const f32x4 val = *reinterpret_cast<const f32x4*>(&tile[px * PS + c * 4]);
            if (px < npx) {
#if defined(PW_ABL) && PW_ABL == 5      // ablation: no output stores
                if (val[0] == 12345.678f)
#endif
                *reinterpret_cast<f32x4*>(dst) = val;
#pragma unroll
                for (int e = 0; e < 4; ++e) { ssum[set][e] += val[e]; ssq[set][e] += val[e] * val[e]; }
            }
        }
    }
    if (tot == nullptr) return;
#if defined(PW_ABL) && PW_ABL == 8      // ablation: sums accumulated, never published
    if (ssum[0][0] != 12345.678f) return;
#endif
    // statistics: scratch [2][COUT][SLOTS]; contributor (wave, set j, lane) of quad (lane + 64 j) % NQ sits in slot (wave * SETS + j) * ceil(64 / NQ) + lane / NQ
    __syncthreads();                          // every wave is done with its tile
    float* const scratch = ic1_lds;
    for (int i = tid; i < 2 * COUT * SLOTS; i += 256) scratch[i] = 0.f;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < SETS; ++j) {
        const int quad = BLOCKED ? j * 4 + (lane & 3) : (lane + 64 * j) % NQ;
        const int slot = BLOCKED ? wave * 16 + (lane >> 2) : (wave * SETS + j) * ((64 + NQ - 1) / NQ) + lane / NQ;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            scratch[(size_t)(quad * 4 + e) * SLOTS + slot] = ssum[j][e];
            scratch[(size_t)(COUT + quad * 4 + e) * SLOTS + slot] = ssq[j][e];
        }
    }
    auto fold = [&](int i) {
        double t = 0;
        for (int l = 0; l < SLOTS; ++l) t += (double)scratch[(size_t)i * SLOTS + l];
        return (float)t;
    };
    stat_word* const acc_lds = reinterpret_cast<stat_word*>(ic1_lds + 4 * 64 * PS);
    stat_publish(tot, b, COUT, bs, rep, blockIdx.x % rep, 0, COUT, fold, acc_lds, tid, 256);
}

template <int COUT, bool BLOCKED>
static hipError_t in_conv1_launch(const float* x, const float* cond, const float* w, const float* bias, float* out,
                                  stat_word* tot, int rep, int bs, int B, int H, int W, hipStream_t s) {
#ifndef IC1_PASSES
#define IC1_PASSES 2
#endif
    const int HW = H * W;
    int per = IC1_PASSES * 256;             // pixels per workgroup (4 waves x 64 pixels per pass), at most 1024 workgroups per sample
    while ((HW + per - 1) / per > 1024) per += 256;
    const int rows = (HW + per - 1) / per;
    constexpr int NQ = COUT / 4, PS = COUT + 4;
    constexpr int G64 = (NQ % 16 == 0) ? 16 : (NQ % 8 == 0) ? 8 : (NQ % 4 == 0) ? 4 : (NQ % 2 == 0) ? 2 : 1;
    constexpr int SLOTS = BLOCKED ? 64 : 4 * (NQ / G64) * ((64 + NQ - 1) / NQ);
    static_assert(2 * COUT * SLOTS <= 4 * 64 * PS, "the statistics scratch aliases the tiles");
    const size_t lds = (size_t)4 * 64 * PS * sizeof(float) + (size_t)(COUT + 2) * STAT_WORDS * sizeof(stat_word) + 16 + (size_t)19 * COUT * sizeof(float);
    {                                       // COUT = 64: 77.7 KB of dynamic LDS
        static int raised[MIDD_MAX_DEVICES] = {};
        hipError_t e = ensure_dynamic_lds(reinterpret_cast<const void*>(&in_conv1_kernel<COUT, BLOCKED>), (int)lds, raised);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((in_conv1_kernel<COUT, BLOCKED>), dim3(rows, B), dim3(256), lds, s, x, cond, w, bias, out, tot, rep, bs, H, W, per);
    return hipGetLastError();
}

hipError_t in_conv_launch(const float* x, const float* cond, const float* w, const float* bias, float* out,
                          stat_word* tot, int rep, int bs, int B, int ic, int H, int W, int Cout, int blocked, hipStream_t s) {
    if (Cout % 16 || Cout / 16 > 256) return hipErrorInvalidValue;
    if (ic == 1 && in_conv1_width(Cout)) {  // the grayscale case: in_conv1_kernel for the widths it is instantiated for
#define MIDD_IC1(N) if (Cout == N) return blocked ? in_conv1_launch<N, true>(x, cond, w, bias, out, tot, rep, bs, B, H, W, s) \
                                                 : in_conv1_launch<N, false>(x, cond, w, bias, out, tot, rep, bs, B, H, W, s);
        MIDD_IC1(48) MIDD_IC1(32) MIDD_IC1(64)
        static_assert(in_conv1_width(48) && in_conv1_width(32) && in_conv1_width(64), "in_conv1_width names the instantiations");
#undef MIDD_IC1
    }
    const int ppi = 256 / (Cout / 16);
    const int rows = pointwise_rows(H * W, ppi);
    const size_t lds = in_conv_lds_bytes(ic, Cout);
    if (lds > POINTWISE_LDS_LIMIT) return hipErrorInvalidValue;      // (mi_unet_plan_create refuses such a network: not reached through the C ABI)
    hipLaunchKernelGGL(in_conv_kernel, dim3(rows, B), dim3(256), lds, s, x, cond, w, bias, out, tot, rep, bs, ic, H, W, Cout, rows, blocked);
    return hipGetLastError();
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

hipError_t out_conv_launch(const OutConvArgs& a, hipStream_t s) {
    if (a.ic > 4 || a.C % 16) return hipErrorInvalidValue;
    const size_t lds = out_conv_dynamic_lds_bytes(a.ic, a.C);
    if (out_conv_lds_bytes(a.ic, a.C) > POINTWISE_LDS_LIMIT) return hipErrorInvalidValue;      // (refused at mi_unet_plan_create)
    const int tiles = ((a.W + OC_T - 1) / OC_T) * ((a.H + OC_T - 1) / OC_T);
    if (a.seeded) {
        if (!a.x || (unsigned long long)a.ic * a.H * a.W >= (1ull << 32) || a.members < 1 || a.v0 < 0) return hipErrorInvalidValue;
        if (a.tiles_x && (a.tiles_x < 1 || a.tiles_y < 1 || a.members != a.tiles_x * a.tiles_y || a.img_H < a.H || a.img_W < a.W ||
                          (unsigned long long)a.ic * a.img_H * a.img_W >= (1ull << 32))) return hipErrorInvalidValue;
        if (a.ic == 1) hipLaunchKernelGGL(out_conv_seeded_kernel<1>, dim3(a.B * tiles), dim3(256), lds, s, a, a.w);
        else hipLaunchKernelGGL(out_conv_seeded_kernel<0>, dim3(a.B * tiles), dim3(256), lds, s, a, a.w);
    } else if (a.ic == 1) hipLaunchKernelGGL(out_conv_kernel<1>, dim3(a.B * tiles), dim3(256), lds, s, a, a.w);
    else hipLaunchKernelGGL(out_conv_kernel<0>, dim3(a.B * tiles), dim3(256), lds, s, a, a.w);
    return hipGetLastError();
}

// a.seeded != 0: the noise term of the slots with SLOT_NOISE is drawn from (a.seed, rec.image, rec.iter, element, member 0); else it
// is read from a.noise when that is given.  a.c1 .. a.c3, a.iter, a.sample_offset, a.v0, a.members and the tile fields are not read.
hipError_t out_conv_slots_launch(const OutConvArgs& a, const SlotRec* slots, hipStream_t s) {
    if (a.ic > 4 || a.C % 16 || !slots || !a.x) return hipErrorInvalidValue;
    if (a.seeded && (a.noise || (unsigned long long)a.ic * a.H * a.W >= (1ull << 32))) return hipErrorInvalidValue;
    const size_t lds = out_conv_dynamic_lds_bytes(a.ic, a.C);
    if (out_conv_lds_bytes(a.ic, a.C) > POINTWISE_LDS_LIMIT) return hipErrorInvalidValue;      // (refused at mi_unet_plan_create)
    const int tiles = ((a.W + OC_T - 1) / OC_T) * ((a.H + OC_T - 1) / OC_T);
    if (a.ic == 1) hipLaunchKernelGGL(out_conv_slots_kernel<1>, dim3(a.B * tiles), dim3(256), lds, s, a, a.w, slots);
    else hipLaunchKernelGGL(out_conv_slots_kernel<0>, dim3(a.B * tiles), dim3(256), lds, s, a, a.w, slots);
    return hipGetLastError();
}

// a.c1 .. a.c3 are not read.  The seeded form is launched only when a term is drawn at all (a.seeded: the host sets it with k.s > 0)
hipError_t out_conv_ddim_launch(const OutConvArgs& a, const DdimCoef& k, hipStream_t s) {
    if (a.ic > 4 || a.C % 16 || !a.x) return hipErrorInvalidValue;
    const size_t lds = out_conv_dynamic_lds_bytes(a.ic, a.C);
    if (out_conv_lds_bytes(a.ic, a.C) > POINTWISE_LDS_LIMIT) return hipErrorInvalidValue;      // (refused at mi_unet_plan_create)
    const int tiles = ((a.W + OC_T - 1) / OC_T) * ((a.H + OC_T - 1) / OC_T);
    if (a.seeded) {
        if (a.noise || (unsigned long long)a.ic * a.H * a.W >= (1ull << 32) || a.members < 1 || a.v0 < 0) return hipErrorInvalidValue;
        if (a.tiles_x && (a.tiles_x < 1 || a.tiles_y < 1 || a.members != a.tiles_x * a.tiles_y || a.img_H < a.H || a.img_W < a.W ||
                          (unsigned long long)a.ic * a.img_H * a.img_W >= (1ull << 32))) return hipErrorInvalidValue;
        if (a.ic == 1) hipLaunchKernelGGL(out_conv_ddim_seeded_kernel<1>, dim3(a.B * tiles), dim3(256), lds, s, a, a.w, k);
        else hipLaunchKernelGGL(out_conv_ddim_seeded_kernel<0>, dim3(a.B * tiles), dim3(256), lds, s, a, a.w, k);
    } else if (a.ic == 1) hipLaunchKernelGGL(out_conv_ddim_kernel<1>, dim3(a.B * tiles), dim3(256), lds, s, a, a.w, k);
    else hipLaunchKernelGGL(out_conv_ddim_kernel<0>, dim3(a.B * tiles), dim3(256), lds, s, a, a.w, k);
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

// ------------------------------------------------------------------------------ ensembles of stochastic samples
// samples [B][K][chw] -> mean [B][chw], unbiased std [B][chw] over the K members of every pixel.  A thread owns V
// neighbouring pixels (V = 4: one 16-byte load per member, 1 KiB per wave instruction, when chw is a multiple of 4 and the
// pointers are 16-byte aligned; V = 1 otherwise) and walks the K member planes chw floats apart, twice (sum; deviations from
// the mean), one load in flight per walk step.  The algorithm needs (K + 2) * 4 bytes per pixel; what the kernel reaches
// against them, at a cache-resident and at a 512 MiB shape, is measured by tools/ensemble_ab.py.
// THE ARITHMETIC IS FIXED (include/midd.h: mi_ensemble_reduce) and per pixel, so neither V nor the grid shows
// in the result: double precision, members in index order, every operation rounded to nearest on its own.  hipcc's
// __dadd_rn / __dmul_rn are the plain operators, which -ffp-contract=fast fuses (q += d * d became one v_fmac_f64), so the
// three operations are functions of this file compiled with contraction off; division and square root are the correctly
// rounded library ones (the FMAs left in the ISA are inside those two).
__device__ __forceinline__ double add_rn64(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double sub_rn64(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double mul_rn64(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}

template <int V>
__global__ __launch_bounds__(256)
void ensemble_reduce_kernel(const float* __restrict__ samples, int K, unsigned long long chw, float* __restrict__ mean, float* __restrict__ stdv) {
    const unsigned long long e = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (e >= chw) return;                                   // (V == 4: chw % 4 == 0, so e + 3 < chw)
    const size_t b = blockIdx.y;
    const float* src = samples + b * (size_t)K * chw + e;
    float x[V];
    auto load = [&](int m) {
        if constexpr (V == 4) { const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)m * chw); x[0] = v.x; x[1] = v.y; x[2] = v.z; x[3] = v.w; }
        else x[0] = src[(size_t)m * chw];
    };
    double sum[V], m64[V];
#pragma unroll
    for (int j = 0; j < V; ++j) sum[j] = 0.0;
    for (int m = 0; m < K; ++m) {
        load(m);
#pragma unroll
        for (int j = 0; j < V; ++j) sum[j] = add_rn64(sum[j], (double)x[j]);
    }
#pragma unroll
    for (int j = 0; j < V; ++j) m64[j] = __ddiv_rn(sum[j], (double)K);
    float out[V];
    if (mean) {
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = __double2float_rn(m64[j]);
        if constexpr (V == 4) *reinterpret_cast<f32x4*>(mean + b * chw + e) = (f32x4){out[0], out[1], out[2], out[3]};
        else mean[b * chw + e] = out[0];
    }
    if (stdv) {
        double q[V];
#pragma unroll
        for (int j = 0; j < V; ++j) q[j] = 0.0;
        for (int m = 0; m < K; ++m) {
            load(m);
#pragma unroll
            for (int j = 0; j < V; ++j) { const double d = sub_rn64((double)x[j], m64[j]); q[j] = add_rn64(q[j], mul_rn64(d, d)); }
        }
#pragma unroll
        for (int j = 0; j < V; ++j) out[j] = __double2float_rn(__dsqrt_rn(__ddiv_rn(q[j], (double)(K - 1))));
        if constexpr (V == 4) *reinterpret_cast<f32x4*>(stdv + b * chw + e) = (f32x4){out[0], out[1], out[2], out[3]};
        else stdv[b * chw + e] = out[0];
    }
}

static inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

hipError_t ensemble_reduce_launch(const float* samples, int B, int K, unsigned long long chw, float* mean, float* stdv, hipStream_t s) {
    if (B < 1 || B > 65535 || K < 1 || chw < 1 || chw >= (1ull << 32) || (!mean && !stdv) || (stdv && K < 2)) return hipErrorInvalidValue;
    if (chw % 4 == 0 && aligned16(samples) && aligned16(mean) && aligned16(stdv))
        hipLaunchKernelGGL(ensemble_reduce_kernel<4>, dim3((unsigned)((chw / 4 + 255) / 256), B), dim3(256), 0, s, samples, K, chw, mean, stdv);
    else
        hipLaunchKernelGGL(ensemble_reduce_kernel<1>, dim3((unsigned)((chw + 255) / 256), B), dim3(256), 0, s, samples, K, chw, mean, stdv);
    return hipGetLastError();
}

// dst [n][chw] <- noisy[(v0 + j) / K]: the condition image of every virtual sample of one ensemble pass (the K members of an
// image share it).  grid (chunks of 256 * V elements, n); 8 bytes per element
template <int V>
__global__ __launch_bounds__(256)
void ensemble_broadcast_kernel(const float* __restrict__ noisy, float* __restrict__ dst, int v0, int K, unsigned long long chw) {
    const unsigned long long e = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (e >= chw) return;
    const size_t j = blockIdx.y, img = (size_t)((unsigned)v0 + blockIdx.y) / (unsigned)K;
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst + j * chw + e) = *reinterpret_cast<const f32x4*>(noisy + img * chw + e);
    else dst[j * chw + e] = noisy[img * chw + e];
}

hipError_t ensemble_broadcast_launch(const float* noisy, float* dst, int v0, int n, int K, unsigned long long chw, hipStream_t s) {
    if (v0 < 0 || n < 1 || n > 65535 || K < 1 || chw < 1 || chw >= (1ull << 32)) return hipErrorInvalidValue;
    if (chw % 4 == 0 && aligned16(noisy) && aligned16(dst))
        hipLaunchKernelGGL(ensemble_broadcast_kernel<4>, dim3((unsigned)((chw / 4 + 255) / 256), n), dim3(256), 0, s, noisy, dst, v0, K, chw);
    else
        hipLaunchKernelGGL(ensemble_broadcast_kernel<1>, dim3((unsigned)((chw + 255) / 256), n), dim3(256), 0, s, noisy, dst, v0, K, chw);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ tiled denoising: extract and blend
// Both are HBM-bound streams over the image (tile_geometry.h holds the geometry; origins come from its formula, no table in
// memory).  Extract: grid (chunks of 256 threads over C * th * tw / V, n virtual samples); the tile is uniform in the
// workgroup, so its origin is scalar arithmetic.  V = 4: a thread moves four neighbouring pixels of one tile row and stores them
// as 16 bytes (tw % 4 == 0, dst 16-byte aligned); it LOADS them as 16 bytes when the source address allows (row pitch W % 4 == 0,
// noisy 16-byte aligned -- `vload` -- and this tile's x0 % 4 == 0), else as four dwords.  V = 1: one dword per thread, any shape.
template <int V>
__global__ __launch_bounds__(256)
void tile_extract_kernel(const float* __restrict__ noisy, float* __restrict__ dst, TileGeom g, int v0, int vload) {
    const unsigned e = (blockIdx.x * 256u + threadIdx.x) * V;                 // element inside the tile block [C][th][tw]
    const unsigned tile_elems = (unsigned)g.C * g.th * g.tw;
    if (e >= tile_elems) return;
    const unsigned v = (unsigned)v0 + blockIdx.y, K = (unsigned)(g.ny * g.nx);
    const unsigned img = v / K, k = v - img * K;
    const int ky = (int)k / g.nx, kx = (int)k - ky * g.nx;
    const int y0 = tile_origin(ky, g.H, g.th, g.ny), x0 = tile_origin(kx, g.W, g.tw, g.nx);
    const unsigned x = e % (unsigned)g.tw, cy = e / (unsigned)g.tw;
    const unsigned y = cy % (unsigned)g.th, c = cy / (unsigned)g.th;
    const float* src = noisy + (((size_t)img * g.C + c) * g.H + (y0 + y)) * (size_t)g.W + x0 + x;
    float* out = dst + (size_t)blockIdx.y * tile_elems + e;
    if constexpr (V == 4) {
        f32x4 r;
        if (vload && (x0 & 3) == 0) r = *reinterpret_cast<const f32x4*>(src);
        else r = (f32x4){src[0], src[1], src[2], src[3]};
        *reinterpret_cast<f32x4*>(out) = r;
    } else {
        *out = *src;
    }
}

hipError_t tile_extract_launch(const float* noisy, float* dst, const TileGeom& g, int v0, int n, hipStream_t s) {
    if (v0 < 0 || n < 1 || n > 65535 || g.C < 1 || g.ny < 1 || g.nx < 1 || g.th < 1 || g.tw < 1 || g.th > g.H || g.tw > g.W ||
        (unsigned long long)g.C * g.th * g.tw >= (1ull << 31)) return hipErrorInvalidValue;
    const unsigned tile_elems = (unsigned)g.C * g.th * g.tw;
    if (g.tw % 4 == 0 && aligned16(dst))
        hipLaunchKernelGGL(tile_extract_kernel<4>, dim3((tile_elems / 4 + 255) / 256, n), dim3(256), 0, s, noisy, dst, g, v0,
                           (g.W % 4 == 0 && aligned16(noisy)) ? 1 : 0);
    else
        hipLaunchKernelGGL(tile_extract_kernel<1>, dim3((tile_elems + 255) / 256, n), dim3(256), 0, s, noisy, dst, g, v0, 0);
    return hipGetLastError();
}

// Blend, as a gather: a thread owns ONE output pixel, finds the tiles that cover it from the origin formula (tile_cover: at most
// three per axis for every geometry the host accepts, but the loop does not rely on it) and walks them in ascending (ky, kx).
// THE ARITHMETIC IS FIXED (include/midd.h: mi_tile_blend) and per pixel: in double, every operation rounded on its own,
//   num += (double)(wy * wx) * (double)v;   den += (double)(wy * wx);   out = (float)(num / den)
// with the integer windows of tile_geometry.h.  No atomics, nothing depends on the launch geometry; a pixel under one tile gets
// that tile's value back exactly (w * v is exact in double, and so is the quotient).  Neighbouring threads read neighbouring
// floats of the same tile row: every wave instruction is a contiguous run (broken once where a tile boundary crosses the wave).
// grid (chunks of 256 pixels of a [C][H][W] block, images -- folded over grid.y when B > 65535)
__global__ __launch_bounds__(256)
void tile_blend_kernel(const float* __restrict__ tiles, float* __restrict__ out, int B, TileGeom g) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (e >= chw) return;
    const int x = (int)(e % (unsigned)g.W);
    const unsigned long long cy = e / (unsigned)g.W;
    const int y = (int)(cy % (unsigned)g.H), c = (int)(cy / (unsigned)g.H);
    int ky0, ky1, kx0, kx1;
    tile_cover(y, g.H, g.th, g.ny, &ky0, &ky1);
    tile_cover(x, g.W, g.tw, g.nx, &kx0, &kx1);
    const size_t tile_plane = (size_t)g.th * g.tw, K = (size_t)g.ny * g.nx;
    for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) {
        double num = 0.0, den = 0.0;
        for (int ky = ky0; ky <= ky1; ++ky) {
            const int ry = y - tile_origin(ky, g.H, g.th, g.ny);
            const int wy = tile_window(ry, g.th, g.oy);
            for (int kx = kx0; kx <= kx1; ++kx) {
                const int rx = x - tile_origin(kx, g.W, g.tw, g.nx);
                const double w = (double)(wy * tile_window(rx, g.tw, g.ox));
                const float v = tiles[((b * K + (size_t)ky * g.nx + kx) * g.C + c) * tile_plane + (size_t)ry * g.tw + rx];
                num = add_rn64(num, mul_rn64(w, (double)v));
                den = add_rn64(den, w);
            }
        }
        out[b * chw + e] = __double2float_rn(__ddiv_rn(num, den));
    }
}

hipError_t tile_blend_launch(const float* tiles, float* out, int B, const TileGeom& g, hipStream_t s) {
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (B < 1 || g.C < 1 || g.ny < 1 || g.nx < 1 || g.th < 1 || g.tw < 1 || g.th > g.H || g.tw > g.W || chw >= (1ull << 32) ||
        g.oy < 0 || g.ox < 0 || (long long)g.oy + 1 > 46340 || (long long)g.ox + 1 > 46340) return hipErrorInvalidValue;      // wy * wx fits an int
    hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)((chw + 255) / 256), B < 65535 ? B : 65535), dim3(256), 0, s, tiles, out, B, g);
    return hipGetLastError();
}

// Blend and reduce in one pass over the image (mi_denoise_tiled_ensemble): tiles [M][B][ny*nx][C][th][tw], the tile outputs of M
// members in run order, -> mean / unbiased std [B][C][H][W] over the members' BLENDED images and, if asked for, those images
// themselves, samples [B][M][C][H][W].  A thread owns ONE output element of one image, as in tile_blend_kernel, whose addressing
// this keeps (member m, image b is the tile block m * B + b).  THE ARITHMETIC IS FIXED (include/midd.h: mi_tile_blend_reduce):
// the composition of the two kernels above, bit for bit --
//   v_m = (float)(num / den) of member m, formed as tile_blend_kernel forms it;  then over v_0 .. v_{M-1}, in index order, the
//   sums of ensemble_reduce_kernel: mean64 = (sum (double)v_m) / M,  q = sum d * d with d = (double)v_m - mean64
// M is a run-time value, so the v_m are not kept: the second walk (std only) blends them again from the tiles -- the same loads
// and the same operations, hence the same bits, whether or not samples is written; nothing is read back from samples.  The
// blended members never exist in memory unless the caller wants them: per pixel (1 or 2) * M * cover tile reads and 1-2 writes,
// against M * cover reads + M writes + 2 * M reads + 2 writes of blend-then-reduce.  No atomics, nothing depends on the grid.
// grid (chunks of 256 elements of a [C][H][W] block, images -- folded over grid.y when B > 65535)
__global__ __launch_bounds__(256)
void tile_blend_reduce_kernel(const float* __restrict__ tiles, float* __restrict__ mean, float* __restrict__ stdv,
                              float* __restrict__ samples, int B, int M, TileGeom g) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (e >= chw) return;
    const int x = (int)(e % (unsigned)g.W);
    const unsigned long long cy = e / (unsigned)g.W;
    const int y = (int)(cy % (unsigned)g.H), c = (int)(cy / (unsigned)g.H);
    int ky0, ky1, kx0, kx1;
    tile_cover(y, g.H, g.th, g.ny, &ky0, &ky1);
    tile_cover(x, g.W, g.tw, g.nx, &kx0, &kx1);
    const size_t tile_plane = (size_t)g.th * g.tw, K = (size_t)g.ny * g.nx;
    for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) {
        auto blended = [&](int m) -> float {                       // tile_blend_kernel's pixel, of tile block m * B + b
            const size_t mb = (size_t)m * B + b;
            double num = 0.0, den = 0.0;
            for (int ky = ky0; ky <= ky1; ++ky) {
                const int ry = y - tile_origin(ky, g.H, g.th, g.ny);
                const int wy = tile_window(ry, g.th, g.oy);
                for (int kx = kx0; kx <= kx1; ++kx) {
                    const int rx = x - tile_origin(kx, g.W, g.tw, g.nx);
                    const double w = (double)(wy * tile_window(rx, g.tw, g.ox));
                    const float v = tiles[((mb * K + (size_t)ky * g.nx + kx) * g.C + c) * tile_plane + (size_t)ry * g.tw + rx];
                    num = add_rn64(num, mul_rn64(w, (double)v));
                    den = add_rn64(den, w);
                }
            }
            return __double2float_rn(__ddiv_rn(num, den));
        };
        double sum = 0.0;
        for (int m = 0; m < M; ++m) {
            const float v = blended(m);
            if (samples) samples[(b * (size_t)M + m) * chw + e] = v;
            sum = add_rn64(sum, (double)v);
        }
        const double m64 = __ddiv_rn(sum, (double)M);
        if (mean) mean[b * chw + e] = __double2float_rn(m64);
        if (stdv) {
            double q = 0.0;
            for (int m = 0; m < M; ++m) {
                const double d = sub_rn64((double)blended(m), m64);
                q = add_rn64(q, mul_rn64(d, d));
            }
            stdv[b * chw + e] = __double2float_rn(__dsqrt_rn(__ddiv_rn(q, (double)(M - 1))));
        }
    }
}

hipError_t tile_blend_reduce_launch(const float* tiles, int B, int M, const TileGeom& g, float* mean, float* stdv, float* samples, hipStream_t s) {
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (B < 1 || M < 1 || g.C < 1 || g.ny < 1 || g.nx < 1 || g.th < 1 || g.tw < 1 || g.th > g.H || g.tw > g.W || chw >= (1ull << 32) ||
        g.oy < 0 || g.ox < 0 || (long long)g.oy + 1 > 46340 || (long long)g.ox + 1 > 46340 ||                          // wy * wx fits an int
        (!mean && !stdv && !samples) || (stdv && M < 2)) return hipErrorInvalidValue;
    const long long BK = (long long)B * ((long long)g.ny * g.nx);            // (ny * nx <= H * W < 2^32: no overflow in either product)
    if (BK > 2147483647ll || BK * M > 2147483647ll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(tile_blend_reduce_kernel, dim3((unsigned)((chw + 255) / 256), B < 65535 ? B : 65535), dim3(256), 0, s,
                       tiles, mean, stdv, samples, B, M, g);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ quantile maps over the members
// samples [B][K][chw] -> out [B][nq][chw]: per pixel the nq quantiles of its K members.  THE ARITHMETIC IS FIXED (include/midd.h:
// mi_ensemble_quantiles) and per pixel, so neither V, the alignment path nor the grid shows in the result: the members are sorted
// by their order keys (quantile_common.h), then per level, in double, every operation rounded on its own,
//   pos = q * (K - 1);  lo = floor(pos);  hi = min(lo + 1, K - 1);  g = pos - lo;  out = (float)(s_lo + g * (s_hi - s_lo))
// A thread owns V neighbouring pixels as ensemble_reduce_kernel does (V = 4: 16-byte loads and stores), loads its K members ONCE,
// keeps the KP >= K keys (K padded to a power of two with keys above +inf) in registers and sorts them with the unrolled network:
// every register index is a compile-time constant.  lo and hi are the same for every pixel (they depend on q and K alone), but
// they are run-time values: s_lo and s_hi are picked by a chain of selects, not by indexing the array, so nothing goes to scratch
// (tests/test_quantiles_cpu.py holds every instantiation to a private segment of 0 bytes).  The levels are kernel arguments.
// A pixel with a NaN member, and a NaN that the interpolation itself makes of infinite members, is the canonical quiet NaN.
struct QuantilePos { int lo, hi; double g; };

__device__ __forceinline__ QuantilePos quantile_pos(double q, int K) {
    const double pos = mul_rn64(q, (double)(K - 1));
    QuantilePos p;
    p.lo = (int)floor(pos);
    p.hi = min(p.lo + 1, K - 1);
    p.g = sub_rn64(pos, (double)p.lo);
    return p;
}

template <int KP>
__device__ __forceinline__ float quantile_of_sorted(const uint32_t (&key)[KP], const QuantilePos& p, int K, bool has_nan) {
    const float s_lo = __uint_as_float(order_bits(pick_key(key, p.lo)));
    const float s_hi = __uint_as_float(order_bits(pick_key(key, p.hi)));
    const float r = __double2float_rn(add_rn64((double)s_lo, mul_rn64(p.g, sub_rn64((double)s_hi, (double)s_lo))));
    const float v = (K == 1) ? s_lo : r;                    // one member: every quantile is that member, bit for bit
    return (has_nan || v != v) ? __uint_as_float(0x7FC00000u) : v;
}

__device__ __forceinline__ bool is_nan_bits(uint32_t bits) { return (bits & 0x7FFFFFFFu) > 0x7F800000u; }

template <int KP, int V>
__global__ __launch_bounds__(256)
void ensemble_quantiles_kernel(const float* __restrict__ samples, int K, unsigned long long chw, QuantileLevels ql, float* __restrict__ out) {
    const unsigned long long e = ((unsigned long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (e >= chw) return;                                   // (V == 4: chw % 4 == 0, so e + 3 < chw)
    const size_t b = blockIdx.y;
    const float* src = samples + b * (size_t)K * chw + e;
    uint32_t key[V][KP];
    bool has_nan[V];
#pragma unroll
    for (int j = 0; j < V; ++j) has_nan[j] = false;
#pragma unroll
    for (int m = 0; m < KP; ++m) {
        if (m < K) {
            uint32_t x[V];
            if constexpr (V == 4) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(src + (size_t)m * chw);
                x[0] = __float_as_uint(v.x); x[1] = __float_as_uint(v.y); x[2] = __float_as_uint(v.z); x[3] = __float_as_uint(v.w);
            } else {
                x[0] = __float_as_uint(src[(size_t)m * chw]);
            }
#pragma unroll
            for (int j = 0; j < V; ++j) { key[j][m] = order_key(x[j]); has_nan[j] = has_nan[j] || is_nan_bits(x[j]); }
        } else {
#pragma unroll
            for (int j = 0; j < V; ++j) key[j][m] = ORDER_KEY_PAD;
        }
    }
#pragma unroll
    for (int j = 0; j < V; ++j) sort_keys<KP>(key[j]);
    float* dst = out + b * (size_t)ql.nq * chw + e;
    for (int i = 0; i < ql.nq; ++i) {
        const QuantilePos p = quantile_pos(ql.q[i], K);
        float r[V];
#pragma unroll
        for (int j = 0; j < V; ++j) r[j] = quantile_of_sorted<KP>(key[j], p, K, has_nan[j]);
        if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst + (size_t)i * chw) = (f32x4){r[0], r[1], r[2], r[3]};
        else dst[(size_t)i * chw] = r[0];
    }
}

static bool quantile_levels_ok(const QuantileLevels& ql) {
    if (ql.nq < 1 || ql.nq > QUANTILE_MAX_LEVELS) return false;
    for (int i = 0; i < ql.nq; ++i)
        if (!(ql.q[i] >= 0.0 && ql.q[i] <= 1.0)) return false;
    return true;
}

template <int KP>
static void ensemble_quantiles_dispatch(const float* samples, int B, int K, unsigned long long chw, const QuantileLevels& ql, float* out, hipStream_t s) {
    if (chw % 4 == 0 && aligned16(samples) && aligned16(out))
        hipLaunchKernelGGL((ensemble_quantiles_kernel<KP, 4>), dim3((unsigned)((chw / 4 + 255) / 256), B), dim3(256), 0, s, samples, K, chw, ql, out);
    else
        hipLaunchKernelGGL((ensemble_quantiles_kernel<KP, 1>), dim3((unsigned)((chw + 255) / 256), B), dim3(256), 0, s, samples, K, chw, ql, out);
}

hipError_t ensemble_quantiles_launch(const float* samples, int B, int K, unsigned long long chw, const QuantileLevels& ql, float* out, hipStream_t s) {
    if (B < 1 || B > 65535 || K < 1 || K > QUANTILE_MAX_MEMBERS || chw < 1 || chw >= (1ull << 32) || !samples || !out || !quantile_levels_ok(ql))
        return hipErrorInvalidValue;
    if (K <= 2) ensemble_quantiles_dispatch<2>(samples, B, K, chw, ql, out, s);
    else if (K <= 4) ensemble_quantiles_dispatch<4>(samples, B, K, chw, ql, out, s);
    else if (K <= 8) ensemble_quantiles_dispatch<8>(samples, B, K, chw, ql, out, s);
    else if (K <= 16) ensemble_quantiles_dispatch<16>(samples, B, K, chw, ql, out, s);
    else if (K <= 32) ensemble_quantiles_dispatch<32>(samples, B, K, chw, ql, out, s);
    else ensemble_quantiles_dispatch<64>(samples, B, K, chw, ql, out, s);
    return hipGetLastError();
}

// Blend and quantiles in one pass over the image (mi_tile_blend_quantiles): tiles [M][B][ny*nx][C][th][tw] -> out [B][nq][C][H][W],
// the quantiles over the members' BLENDED images, which never exist in memory.  A thread owns ONE output element of one image
// with the addressing of tile_blend_reduce_kernel.  THE ARITHMETIC IS FIXED: v_m = (float)(num_m / den) exactly as
// tile_blend_kernel forms it -- the covering tiles in ascending (ky, kx), num_m += (double)(wy * wx) * (double)v -- for every member
// once, then the sort and the interpolation of ensemble_quantiles_kernel over v_0 .. v_{M-1}: the output equals mi_tile_blend of
// every member followed by mi_ensemble_quantiles, bit for bit.  The tile walk is the outer loop and the members the unrolled inner
// one: the windows are formed once per tile, a tile's M loads are in flight together, and every member still sees its own
// additions in the same order (den is the same sum for every member).  KP doubles and KP keys per thread, all at constant indices.
// grid (chunks of 256 elements of a [C][H][W] block, images -- folded over grid.y when B > 65535)
template <int KP>
__global__ __launch_bounds__(256)
void tile_blend_quantiles_kernel(const float* __restrict__ tiles, float* __restrict__ out, int B, int M, TileGeom g, QuantileLevels ql) {
    const unsigned long long e = (unsigned long long)blockIdx.x * 256 + threadIdx.x;
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (e >= chw) return;
    const int x = (int)(e % (unsigned)g.W);
    const unsigned long long cy = e / (unsigned)g.W;
    const int y = (int)(cy % (unsigned)g.H), c = (int)(cy / (unsigned)g.H);
    int ky0, ky1, kx0, kx1;
    tile_cover(y, g.H, g.th, g.ny, &ky0, &ky1);
    tile_cover(x, g.W, g.tw, g.nx, &kx0, &kx1);
    const size_t tile_plane = (size_t)g.th * g.tw, K = (size_t)g.ny * g.nx;
    const size_t member_stride = (size_t)B * K * g.C * tile_plane;             // tile block m * B + b: m * member_stride further on
    for (size_t b = blockIdx.y; b < (size_t)B; b += gridDim.y) {
        double num[KP], den = 0.0;
#pragma unroll
        for (int m = 0; m < KP; ++m) num[m] = 0.0;
        for (int ky = ky0; ky <= ky1; ++ky) {
            const int ry = y - tile_origin(ky, g.H, g.th, g.ny);
            const int wy = tile_window(ry, g.th, g.oy);
            for (int kx = kx0; kx <= kx1; ++kx) {
                const int rx = x - tile_origin(kx, g.W, g.tw, g.nx);
                const double w = (double)(wy * tile_window(rx, g.tw, g.ox));
                const float* src = tiles + ((b * K + (size_t)ky * g.nx + kx) * g.C + c) * tile_plane + (size_t)ry * g.tw + rx;
#pragma unroll
                for (int m = 0; m < KP; ++m)
                    if (m < M) num[m] = add_rn64(num[m], mul_rn64(w, (double)src[(size_t)m * member_stride]));
                den = add_rn64(den, w);
            }
        }
        uint32_t key[KP];
        bool has_nan = false;
#pragma unroll
        for (int m = 0; m < KP; ++m) {
            if (m < M) {
                const uint32_t bits = __float_as_uint(__double2float_rn(__ddiv_rn(num[m], den)));
                key[m] = order_key(bits);
                has_nan = has_nan || is_nan_bits(bits);
            } else {
                key[m] = ORDER_KEY_PAD;
            }
        }
        sort_keys<KP>(key);
        float* dst = out + b * (size_t)ql.nq * chw + e;
        for (int i = 0; i < ql.nq; ++i) dst[(size_t)i * chw] = quantile_of_sorted<KP>(key, quantile_pos(ql.q[i], M), M, has_nan);
    }
}

hipError_t tile_blend_quantiles_launch(const float* tiles, int B, int M, const TileGeom& g, const QuantileLevels& ql, float* out, hipStream_t s) {
    const unsigned long long chw = (unsigned long long)g.C * g.H * g.W;
    if (B < 1 || M < 1 || M > QUANTILE_MAX_MEMBERS || g.C < 1 || g.ny < 1 || g.nx < 1 || g.th < 1 || g.tw < 1 || g.th > g.H || g.tw > g.W ||
        chw >= (1ull << 32) || g.oy < 0 || g.ox < 0 || (long long)g.oy + 1 > 46340 || (long long)g.ox + 1 > 46340 ||      // wy * wx fits an int
        !tiles || !out || !quantile_levels_ok(ql)) return hipErrorInvalidValue;
    const long long BK = (long long)B * ((long long)g.ny * g.nx);            // (ny * nx <= H * W < 2^32: no overflow in either product)
    if (BK > 2147483647ll || BK * M > 2147483647ll) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((chw + 255) / 256), B < 65535 ? B : 65535);
#define MIDD_TBQ(N) hipLaunchKernelGGL(tile_blend_quantiles_kernel<N>, grid, dim3(256), 0, s, tiles, out, B, M, g, ql)
    if (M <= 2) MIDD_TBQ(2);
    else if (M <= 4) MIDD_TBQ(4);
    else if (M <= 8) MIDD_TBQ(8);
    else if (M <= 16) MIDD_TBQ(16);
    else if (M <= 32) MIDD_TBQ(32);
    else MIDD_TBQ(64);
#undef MIDD_TBQ
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ geometric self-ensemble: the 8 flip / rotate views
// THE GEOMETRY IS FIXED (include/midd.h): view code g = 4 t + 2 fy + fx on the last two axes of a [C][H][W] image,
//   non-transposing (t = 0):  view(x)[p][q] = x[fy ? H-1-p : p][fx ? W-1-q : q]     and unview is the same map (an involution)
//   transposing (t = 1, H == W == N):  view(x)[p][q] = x[fx ? N-1-q : q][fy ? N-1-p : p],  unview(v)[p][q] = v[fy ? N-1-q : q][fx ? N-1-p : p]
// so every direction is ONE gather  dst[p][q] = src[rr ? .. q : q][rc ? .. p : p]  (transposing) or  src[rr ? .. p][rc ? .. q]  (not),
// with (rr, rc) = (fy, fx) except for the transposing view() itself, where they swap.  All of it is data movement: bit copies.
// A workgroup of 256 threads owns a DH_T x DH_T (32 x 32) tile of one [H][W] plane of the destination; thread (r = tid / 8,
// c = tid % 8) owns the four neighbouring pixels (p0 + r, q0 + 4 c ..+3).  Not transposing, a thread's quad is a quad of one source
// row, read in place (reversed inside the quad when rc): no LDS.  Transposing, the quad is a piece of a source COLUMN, one float per
// 4 N bytes: the workgroup reads the transposed source tile row by row instead (thread (r, c): source row of q0 + r, the quad of
// columns of p0 + 4 c ..+3: 128 contiguous bytes per 8 lanes, whole lines) into an LDS patch [q - q0][p - p0] of pitch 33 words --
// the reversals are applied on the way in, so the patch is in destination coordinates -- and after one barrier reads its pixels
// from patch[4 c + j][r]: with pitch 33 both the stores (bank r + 4 c + j) and the loads (bank 4 c + j + r) of a 32-lane group hit 32
// different banks.  `vec`: the quads move as 16 bytes (W % 4 == 0, every pointer 16-byte aligned: then a quad never crosses the
// right edge and every quad start, reversed or not, is a multiple of 4); else dword by dword with bounds checks -- the same values.
constexpr int DH_T = 32, DH_PITCH = DH_T + 1, DH_PATCH = DH_T * DH_PITCH;

struct DihedralTile { int p0, q0, c; };
__device__ __forceinline__ DihedralTile dihedral_tile(int H, int W) {
    const unsigned tiles_q = (unsigned)(W + DH_T - 1) / DH_T, tiles_p = (unsigned)(H + DH_T - 1) / DH_T;
    const unsigned tq = blockIdx.x % tiles_q, rest = blockIdx.x / tiles_q;
    return DihedralTile{(int)(rest % tiles_p) * DH_T, (int)tq * DH_T, (int)(rest / tiles_p)};
}

// out[j] <- src[rr ? H-1-p : p][rc ? W-1-(q+j) : q+j], j = 0..3, for the pixels inside the plane (the others keep their value)
__device__ __forceinline__ void dihedral_quad_direct(const float* __restrict__ src, int H, int W, int p, int q, bool rr, bool rc, int vec, float (&out)[4]) {
    if (p >= H || q >= W) return;
    const float* row = src + (size_t)(rr ? H - 1 - p : p) * W;
    if (vec) {
        const f32x4 v = *reinterpret_cast<const f32x4*>(row + (rc ? W - 4 - q : q));
        out[0] = rc ? v.w : v.x; out[1] = rc ? v.z : v.y; out[2] = rc ? v.y : v.z; out[3] = rc ? v.x : v.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q + j < W) out[j] = row[rc ? W - 1 - (q + j) : q + j];
    }
}

// patch[q - q0][p - p0] <- src[rr ? N-1-q : q][rc ? N-1-p : p] for the tile's pixels inside the N x N plane (all 256 threads call it)
__device__ __forceinline__ void dihedral_stage_transposed(const float* __restrict__ src, int N, int p0, int q0, bool rr, bool rc, int vec, float* patch) {
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    dihedral_quad_direct(src, N, N, q0 + r, p0 + c4, rr, rc, vec, v);        // (the source tile is a non-transposing gather at (q0, p0))
    if (q0 + r < N) {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (p0 + c4 + j < N) patch[r * DH_PITCH + c4 + j] = v[j];
    }
}

__device__ __forceinline__ void dihedral_quad_from_patch(const float* patch, float (&out)[4]) {
    const int r = threadIdx.x >> 3, c4 = (threadIdx.x & 7) * 4;
#pragma unroll
    for (int j = 0; j < 4; ++j) out[j] = patch[(c4 + j) * DH_PITCH + r];     // (words outside the plane hold stale LDS: never stored to memory)
}

__device__ __forceinline__ void dihedral_store_quad(float* __restrict__ dst, int W, int p, int q, int vec, const float (&v)[4]) {
    float* o = dst + (size_t)p * W + q;
    if (vec) *reinterpret_cast<f32x4*>(o) = (f32x4){v[0], v[1], v[2], v[3]};
    else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (q + j < W) o[j] = v[j];
    }
}

// The fill: dst [n][C][Hv][Wv] <- view(images[(v0 + j) / G], code[(v0 + j) % G]) for the n virtual samples from v0 (image-major).
// grid (tiles of a view's plane * C, n); the code is uniform in the workgroup, so only workgroups of a transposing view touch LDS.
__global__ __launch_bounds__(256)
void dihedral_views_kernel(const float* __restrict__ images, float* __restrict__ dst, DihedralViews dv, int C, int H, int W, int v0, int vec) {
    __shared__ float patch[DH_PATCH];
    const unsigned v = (unsigned)v0 + blockIdx.y, G = (unsigned)dv.n;
    const unsigned img = v / G, code = dv.code[v - img * G];
    const bool t = code & 4, fy = code & 2, fx = code & 1;
    const DihedralTile tl = dihedral_tile(H, W);                              // (t: H == W, the view's plane has the image's shape)
    const size_t plane = (size_t)H * W;
    const float* src = images + ((size_t)img * C + tl.c) * plane;
    const int p = tl.p0 + (threadIdx.x >> 3), q = tl.q0 + (threadIdx.x & 7) * 4;
    float x[4] = {0.f, 0.f, 0.f, 0.f};
    if (t) {
        dihedral_stage_transposed(src, H, tl.p0, tl.q0, fx, fy, vec, patch);
        __syncthreads();
        dihedral_quad_from_patch(patch, x);
    } else {
        dihedral_quad_direct(src, H, W, p, q, fy, fx, vec, x);
    }
    if (p < H && q < W) dihedral_store_quad(dst + ((size_t)blockIdx.y * C + tl.c) * plane, W, p, q, vec, x);
}

static bool dihedral_views_ok(const DihedralViews& dv, int C, int H, int W, unsigned* grid_x) {
    if (dv.n < 1 || dv.n > DIHEDRAL_MAX_VIEWS || C < 1 || H < 1 || W < 1 || (unsigned long long)C * H * W >= (1ull << 32)) return false;
    for (int k = 0; k < dv.n; ++k)
        if (dv.code[k] > 7 || ((dv.code[k] & 4) && H != W)) return false;
    const unsigned long long blocks = (unsigned long long)((H + DH_T - 1) / DH_T) * ((W + DH_T - 1) / DH_T) * C;
    if (blocks > 2147483647ull) return false;
    *grid_x = (unsigned)blocks;
    return true;
}

static bool dihedral_transposes(const DihedralViews& dv) {
    for (int k = 0; k < dv.n; ++k)
        if (dv.code[k] & 4) return true;
    return false;
}

hipError_t dihedral_views_launch(const float* images, float* dst, const DihedralViews& dv, int C, int H, int W, int v0, int n, hipStream_t s) {
    unsigned gx = 0;
    if (!dihedral_views_ok(dv, C, H, W, &gx) || v0 < 0 || n < 1 || n > 65535 || !images || !dst) return hipErrorInvalidValue;
    const int vec = (W % 4 == 0 && ((size_t)H * W) % 4 == 0 && aligned16(images) && aligned16(dst)) ? 1 : 0;
    hipLaunchKernelGGL(dihedral_views_kernel, dim3(gx, n), dim3(256), 0, s, images, dst, dv, C, H, W, v0, vec);
    return hipGetLastError();
}

// The members of a thread's four pixels, turned back into the image's frame: x[k][j] = unview(views_out[b][k], code[k]) at the
// pixel, k = 0 .. G-1 in list order, in registers (the loop over the 8 possible views is unrolled: every index is a constant).
// TR (some view of the list transposes): every transposing view of the list gets an LDS patch of its own (at most four codes
// transpose), all are staged, ONE barrier, then every thread picks its pixels up.  !TR: no LDS, no barrier.
template <bool TR>
__device__ __forceinline__ void dihedral_gather_members(const float* __restrict__ views_b, const DihedralViews& dv, const DihedralTile& tl,
                                                        int C, int H, int W, int vec, float* patches, float (&x)[DIHEDRAL_MAX_VIEWS][4]) {
    const size_t plane = (size_t)H * W;
    const int p = tl.p0 + (threadIdx.x >> 3), q = tl.q0 + (threadIdx.x & 7) * 4;
    if constexpr (TR) {
        int slot = 0;
#pragma unroll
        for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k)
            if (k < dv.n && (dv.code[k] & 4)) {
                dihedral_stage_transposed(views_b + ((size_t)k * C + tl.c) * plane, H, tl.p0, tl.q0, dv.code[k] & 2, dv.code[k] & 1, vec,
                                          patches + slot * DH_PATCH);
                ++slot;
            }
        __syncthreads();
    }
    int slot = 0;
#pragma unroll
    for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k) {
#pragma unroll
        for (int j = 0; j < 4; ++j) x[k][j] = 0.f;
        if (k < dv.n) {
            if (TR && (dv.code[k] & 4)) {
                dihedral_quad_from_patch(patches + slot * DH_PATCH, x[k]);
                ++slot;
            } else {
                dihedral_quad_direct(views_b + ((size_t)k * C + tl.c) * plane, H, W, p, q, dv.code[k] & 2, dv.code[k] & 1, vec, x[k]);
            }
        }
    }
}

// The final launch of mi_denoise_self_ensemble: views_out [B][G][C][Hv][Wv], the sampler outputs in each view's own frame, ->
// mean / unbiased std [B][C][H][W] over the G views turned back and, if asked for, those aligned members [B][G][C][H][W].
// THE ARITHMETIC IS FIXED (include/midd.h: mi_dihedral_reduce): the gather above, then exactly ensemble_reduce_kernel's sums over
// x_0 .. x_{G-1} in list order -- the result equals unview per view followed by mi_ensemble_reduce, bit for bit, with or without
// `samples`; the aligned members exist in memory only when the caller wants them.  grid (tiles of a plane * C, B)
template <bool TR>
__global__ __launch_bounds__(256)
void dihedral_reduce_kernel(const float* __restrict__ views_out, float* __restrict__ mean, float* __restrict__ stdv, float* __restrict__ samples,
                            DihedralViews dv, int C, int H, int W, int vec) {
    __shared__ float patches[TR ? 4 * DH_PATCH : 1];
    const DihedralTile tl = dihedral_tile(H, W);
    const size_t b = blockIdx.y, plane = (size_t)H * W, chw = (size_t)C * plane;
    const int G = dv.n;
    float x[DIHEDRAL_MAX_VIEWS][4];
    dihedral_gather_members<TR>(views_out + b * G * chw, dv, tl, C, H, W, vec, patches, x);
    const int p = tl.p0 + (threadIdx.x >> 3), q = tl.q0 + (threadIdx.x & 7) * 4;
    if (p >= H || q >= W) return;                            // (after the barrier)
    const size_t at = b * chw + (size_t)tl.c * plane;        // the pixel's [H][W] plane inside a [B][C][H][W] output
    double sum[4], m64[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sum[j] = 0.0;
#pragma unroll
    for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k)
        if (k < G) {
            if (samples) dihedral_store_quad(samples + (b * G + k) * chw + (size_t)tl.c * plane, W, p, q, vec, x[k]);
#pragma unroll
            for (int j = 0; j < 4; ++j) sum[j] = add_rn64(sum[j], (double)x[k][j]);
        }
    float out[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { m64[j] = __ddiv_rn(sum[j], (double)G); out[j] = __double2float_rn(m64[j]); }
    if (mean) dihedral_store_quad(mean + at, W, p, q, vec, out);
    if (stdv) {
        double dev[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) dev[j] = 0.0;
#pragma unroll
        for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k)
            if (k < G) {
#pragma unroll
                for (int j = 0; j < 4; ++j) { const double d = sub_rn64((double)x[k][j], m64[j]); dev[j] = add_rn64(dev[j], mul_rn64(d, d)); }
            }
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = __double2float_rn(__dsqrt_rn(__ddiv_rn(dev[j], (double)(G - 1))));
        dihedral_store_quad(stdv + at, W, p, q, vec, out);
    }
}

hipError_t dihedral_reduce_launch(const float* views_out, int B, const DihedralViews& dv, int C, int H, int W,
                                  float* mean, float* stdv, float* samples, hipStream_t s) {
    unsigned gx = 0;
    if (!dihedral_views_ok(dv, C, H, W, &gx) || B < 1 || B > 65535 || !views_out || (!mean && !stdv && !samples) || (stdv && dv.n < 2))
        return hipErrorInvalidValue;
    const int vec = (W % 4 == 0 && ((size_t)H * W) % 4 == 0 && aligned16(views_out) && aligned16(mean) && aligned16(stdv) && aligned16(samples)) ? 1 : 0;
    if (dihedral_transposes(dv))
        hipLaunchKernelGGL(dihedral_reduce_kernel<true>, dim3(gx, B), dim3(256), 0, s, views_out, mean, stdv, samples, dv, C, H, W, vec);
    else
        hipLaunchKernelGGL(dihedral_reduce_kernel<false>, dim3(gx, B), dim3(256), 0, s, views_out, mean, stdv, samples, dv, C, H, W, vec);
    return hipGetLastError();
}

// views_out [B][G][C][Hv][Wv] -> out [B][nq][C][H][W]: the gather above, then the sort and the interpolation of
// ensemble_quantiles_kernel over x_0 .. x_{G-1} (G <= 8: the one network of 8 keys): mi_ensemble_quantiles of the aligned members,
// bit for bit, which never exist in memory.  Keys and members at constant register indices only: no scratch.  grid as above
template <bool TR>
__global__ __launch_bounds__(256)
void dihedral_quantiles_kernel(const float* __restrict__ views_out, float* __restrict__ out, DihedralViews dv, QuantileLevels ql,
                               int C, int H, int W, int vec) {
    __shared__ float patches[TR ? 4 * DH_PATCH : 1];
    const DihedralTile tl = dihedral_tile(H, W);
    const size_t b = blockIdx.y, plane = (size_t)H * W, chw = (size_t)C * plane;
    const int G = dv.n;
    float x[DIHEDRAL_MAX_VIEWS][4];
    dihedral_gather_members<TR>(views_out + b * G * chw, dv, tl, C, H, W, vec, patches, x);
    const int p = tl.p0 + (threadIdx.x >> 3), q = tl.q0 + (threadIdx.x & 7) * 4;
    if (p >= H || q >= W) return;                            // (after the barrier)
    uint32_t key[4][DIHEDRAL_MAX_VIEWS];
    bool has_nan[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        has_nan[j] = false;
#pragma unroll
        for (int k = 0; k < DIHEDRAL_MAX_VIEWS; ++k) {
            const uint32_t bits = __float_as_uint(x[k][j]);
            key[j][k] = (k < G) ? order_key(bits) : ORDER_KEY_PAD;
            has_nan[j] = has_nan[j] || (k < G && is_nan_bits(bits));
        }
        sort_keys<DIHEDRAL_MAX_VIEWS>(key[j]);
    }
    float* dst = out + b * (size_t)ql.nq * chw + (size_t)tl.c * plane;
    for (int i = 0; i < ql.nq; ++i) {
        const QuantilePos pos = quantile_pos(ql.q[i], G);
        float r[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) r[j] = quantile_of_sorted<DIHEDRAL_MAX_VIEWS>(key[j], pos, G, has_nan[j]);
        dihedral_store_quad(dst + (size_t)i * chw, W, p, q, vec, r);
    }
}

hipError_t dihedral_quantiles_launch(const float* views_out, int B, const DihedralViews& dv, int C, int H, int W,
                                     const QuantileLevels& ql, float* out, hipStream_t s) {
    unsigned gx = 0;
    if (!dihedral_views_ok(dv, C, H, W, &gx) || B < 1 || B > 65535 || !views_out || !out || !quantile_levels_ok(ql)) return hipErrorInvalidValue;
    const int vec = (W % 4 == 0 && ((size_t)H * W) % 4 == 0 && aligned16(views_out) && aligned16(out)) ? 1 : 0;
    if (dihedral_transposes(dv))
        hipLaunchKernelGGL(dihedral_quantiles_kernel<true>, dim3(gx, B), dim3(256), 0, s, views_out, out, dv, ql, C, H, W, vec);
    else
        hipLaunchKernelGGL(dihedral_quantiles_kernel<false>, dim3(gx, B), dim3(256), 0, s, views_out, out, dv, ql, C, H, W, vec);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ bilinear resize (NHWC; the channel-blocked variant follows)
// Same index/weight arithmetic as ATen's upsample_bilinear2d with align_corners=False:
//   src = max(0, scale*(dst+0.5)-0.5), scale = in/out;  i0 = floor(src), i1 = i0 + (i0 < in-1), l1 = src - i0.
// grid (rows, B); also leaves the GroupNorm totals of its output (pointwise_publish)
__global__ __launch_bounds__(256)
void resize_bilinear_kernel(const float* __restrict__ src, float* __restrict__ dst, stat_word* __restrict__ tot, int rep, int bs,
                            int H, int W, int C, int OH, int OW, float sy, float sx, int rows) {
    extern __shared__ float rs_lds[];             // statistics scratch
    const int CQ = C >> 2;
    const int ppi = 256 / CQ;
    const int tid = threadIdx.x;
    const int pl = tid / CQ, cq = tid - pl * CQ;
    const bool active = pl < ppi;
    const int b = blockIdx.y, row = blockIdx.x;
    const int OHW = OH * OW;
    const int per = (OHW + rows - 1) / rows;
    const int p0 = row * per, p1 = min(OHW, p0 + per);
    float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
    if (active) {
        const float* base = src + (size_t)b * H * W * C + cq * 4;
        for (int p = p0 + pl; p < p1; p += ppi) {
            const int oy = p / OW, ox = p - oy * OW;
            float fy = sy * ((float)oy + 0.5f) - 0.5f; if (fy < 0.f) fy = 0.f;
            float fx = sx * ((float)ox + 0.5f) - 0.5f; if (fx < 0.f) fx = 0.f;
            const int y0 = (int)fy, x0 = (int)fx;
            const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
            const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
            const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
            const f32x4 v00 = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * W + x0) * C);
            const f32x4 v01 = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * W + x1) * C);
            const f32x4 v10 = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * W + x0) * C);
            const f32x4 v11 = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * W + x1) * C);
            const f32x4 r = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
            *reinterpret_cast<f32x4*>(dst + ((size_t)b * OHW + p) * C + cq * 4) = r;
#pragma unroll
            for (int e = 0; e < 4; ++e) { ssum[e] += r[e]; ssq[e] += r[e] * r[e]; }
        }
    }
    if (tot == nullptr) return;
    stat_word* const acc_lds = reinterpret_cast<stat_word*>(rs_lds + 2 * (size_t)C * ppi);       // C % 4 == 0: 8-byte aligned
    pointwise_publish<4>(ssum, ssq, active, pl, ppi, cq, C, rs_lds, acc_lds, tot, b, bs, rep, row % rep, tid);
}

// Channel-blocked tensors [B][C/16][H][W][16] (midd_internal.h): grid (rows, B, C/16), thread = (pixel lane 0..63, quad 0..3 of
// the block) -- a wave reads and writes whole contiguous runs of 16 pixels x 64 bytes.  Same arithmetic and statistics as above.
__global__ __launch_bounds__(256)
void resize_bilinear_blocked_kernel(const float* __restrict__ src, float* __restrict__ dst, stat_word* __restrict__ tot, int rep, int bs,
                                    int H, int W, int C, int OH, int OW, float sy, float sx, int rows) {
    __shared__ float rs_scratch[2 * 16 * 64];
    __shared__ stat_word rs_acc[(16 + 2) * STAT_WORDS];
    const int tid = threadIdx.x;
    const int pl = tid >> 2, q = tid & 3;
    const int b = blockIdx.y, row = blockIdx.x, blk = blockIdx.z;
    const int OHW = OH * OW;
    const int per = (OHW + rows - 1) / rows;
    const int p0 = row * per, p1 = min(OHW, p0 + per);
    float ssum[4] = {0.f, 0.f, 0.f, 0.f}, ssq[4] = {0.f, 0.f, 0.f, 0.f};
    const float* base = src + (((size_t)b * (C >> 4) + blk) * (size_t)(H * W)) * 16 + q * 4;
    float* const obase = dst + (((size_t)b * (C >> 4) + blk) * (size_t)OHW) * 16 + q * 4;
    for (int p = p0 + pl; p < p1; p += 64) {
        const int oy = p / OW, ox = p - oy * OW;
        float fy = sy * ((float)oy + 0.5f) - 0.5f; if (fy < 0.f) fy = 0.f;
        float fx = sx * ((float)ox + 0.5f) - 0.5f; if (fx < 0.f) fx = 0.f;
        const int y0 = (int)fy, x0 = (int)fx;
        const int y1 = y0 + (y0 < H - 1 ? 1 : 0), x1 = x0 + (x0 < W - 1 ? 1 : 0);
        const float ly1 = fy - (float)y0, lx1 = fx - (float)x0;
        const float ly0 = 1.0f - ly1, lx0 = 1.0f - lx1;
        const f32x4 v00 = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * W + x0) * 16);
        const f32x4 v01 = *reinterpret_cast<const f32x4*>(base + ((size_t)y0 * W + x1) * 16);
        const f32x4 v10 = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * W + x0) * 16);
        const f32x4 v11 = *reinterpret_cast<const f32x4*>(base + ((size_t)y1 * W + x1) * 16);
        const f32x4 r = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11);
        *reinterpret_cast<f32x4*>(obase + (size_t)p * 16) = r;
#pragma unroll
        for (int e = 0; e < 4; ++e) { ssum[e] += r[e]; ssq[e] += r[e] * r[e]; }
    }
    if (tot == nullptr) return;
    pointwise_publish<4>(ssum, ssq, true, pl, 64, q, C, rs_scratch, rs_acc, tot, b, bs, rep, row % rep, tid, 256, blk * 16, 16);
}

hipError_t resize_bilinear_launch(const float* src, float* dst, stat_word* tot, int rep, int bs, int B, int H, int W, int C, int OH, int OW, int blocked, hipStream_t s) {
    if (blocked) {
        if (C % 16) return hipErrorInvalidValue;
        const int rows_b = pointwise_rows(OH * OW, 64);
        hipLaunchKernelGGL(resize_bilinear_blocked_kernel, dim3(rows_b, B, C / 16), dim3(256), 0, s,
                           src, dst, tot, rep, bs, H, W, C, OH, OW, (float)H / (float)OH, (float)W / (float)OW, rows_b);
        return hipGetLastError();
    }
    if (C % 4 || C / 4 > 256) return hipErrorInvalidValue;
    const int ppi = 256 / (C / 4);
    const int rows = pointwise_rows(OH * OW, ppi);
    const size_t lds = (size_t)2 * C * ppi * sizeof(float) + (size_t)(C + 2) * STAT_WORDS * sizeof(stat_word);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resize_bilinear_kernel, dim3(rows, B), dim3(256), lds, s,
                       src, dst, tot, rep, bs, H, W, C, OH, OW, (float)H / (float)OH, (float)W / (float)OW, rows);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ ConvTranspose2d(4,2,1) direct
// out[oy][ox][co] = bias[co] + sum_{ky,kx,ci} in[(oy+1-ky)/2][(ox+1-kx)/2][ci] * w[ky][kx][ci][co]
// over taps with (oy+1-ky), (ox+1-kx) even and in range.  Thread = (output pixel, 4 couts).
__global__ __launch_bounds__(256)
void conv_transpose_kernel(const float* __restrict__ src, const float* __restrict__ w, const float* __restrict__ bias,
                           float* __restrict__ dst, int B, int H, int W, int Cin, int Cout, int blocked) {
    const int OH = 2 * H, OW = 2 * W, CQ = Cout >> 2;
    const long total = (long)B * OH * OW * CQ;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int cq = (int)(gid % CQ);
    const long pix = gid / CQ;
    const int ox = (int)(pix % OW);
    const int oy = (int)((pix / OW) % OH);
    const int b = (int)(pix / ((long)OW * OH));
    f32x4 acc = *reinterpret_cast<const f32x4*>(bias + cq * 4);
    for (int ky = 0; ky < 4; ++ky) {
        const int ny = oy + 1 - ky;
        if (ny < 0 || (ny & 1) || (ny >> 1) >= H) continue;
        for (int kx = 0; kx < 4; ++kx) {
            const int nx = ox + 1 - kx;
            if (nx < 0 || (nx & 1) || (nx >> 1) >= W) continue;
            const int ipix = (ny >> 1) * W + (nx >> 1);
            const float* wp = w + ((size_t)(ky * 4 + kx) * Cin) * Cout + cq * 4;
            for (int ci = 0; ci < Cin; ++ci)
                acc += src[act_index(blocked, b, Cin, H * W, ipix, ci)] * *reinterpret_cast<const f32x4*>(wp + (size_t)ci * Cout);
        }
    }
    *reinterpret_cast<f32x4*>(dst + act_index(blocked, b, Cout, OH * OW, oy * OW + ox, cq * 4)) = acc;
}

hipError_t conv_transpose_launch(const float* src, const float* w, const float* bias, float* dst,
                                 int B, int H, int W, int Cin, int Cout, int blocked, hipStream_t s) {
    if (Cout % 4) return hipErrorInvalidValue;
    const long total = (long)B * 4 * H * W * (Cout / 4);
    hipLaunchKernelGGL(conv_transpose_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s,
                       src, w, bias, dst, B, H, W, Cin, Cout, blocked);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------ helpers
__global__ void nhwc_to_nchw_kernel(const float* __restrict__ src, float* __restrict__ dst, int B, int H, int W, int C, int blocked) {
    const long total = (long)B * H * W * C;
    const long gid = (long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= total) return;
    const int c = (int)(gid % C);
    const long pix = gid / C;
    const long hw = pix % ((long)H * W);
    const int b = (int)(pix / ((long)H * W));
    dst[((size_t)b * C + c) * H * W + hw] = src[act_index(blocked, b, C, H * W, (int)hw, c)];
}

hipError_t nhwc_to_nchw_launch(const float* src, float* dst, int B, int H, int W, int C, int blocked, hipStream_t s) {
    const long total = (long)B * H * W * C;
    hipLaunchKernelGGL(nhwc_to_nchw_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, src, dst, B, H, W, C, blocked);
    return hipGetLastError();
}

struct I32x32 { int v[32]; };
__global__ void fill_i32_kernel(int* dst, I32x32 vals, int n) {
    if ((int)threadIdx.x < n) dst[threadIdx.x] = vals.v[threadIdx.x];
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

hipError_t fill_i32_launch(int* dst, const int* host_vals, int n, hipStream_t s) {
    for (int i = 0; i < n; i += 32) {
        I32x32 v;
        const int m = (n - i < 32) ? n - i : 32;
        for (int j = 0; j < 32; ++j) v.v[j] = (j < m) ? host_vals[i + j] : 0;
        hipLaunchKernelGGL(fill_i32_kernel, dim3(1), dim3(32), 0, s, dst + i, v, m);
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

}  // namespace midd
