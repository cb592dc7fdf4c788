// The HBM-bound direct kernel at the head of the UNet.
//
//   in_conv_kernel   : Conv3x3(cat[x, condition]) 2*ic -> Cout        (DDIMModel.py:222-223)
//   in_conv1_kernel  : the same for one image channel, the reference's grayscale case
// K = 18 is a degenerate GEMM shape: it stays on the vector ALU and is judged against the HBM roofline.
#include "midd_internal.h"
#include "pointwise_common.h"

namespace midd {

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

}  // namespace midd
