// Implicit-GEMM convolution with fp32 operands SPLIT into two fp16 halves and three
// v_mfma_f32_16x16x32_f16 products per K-step ("f16x3"), fp32 accumulation, for gfx950.
//
// Why: the fp32-input MFMA runs at 1/16 of the fp16 rate (MI355X_MICROARCH.md); fp16 x fp16
// products are exact in the fp32 accumulator, so with the exact power-of-two prescales
//     x' = x * 2^s :  x' = xh + xl,   xh = fp16(x'),  xl = fp16(x' - xh)       (|err| <= 2^-22 |x'|)
//     w' = w * 2^k :  w' = wh + wl    (k per layer so that max|w'| ~ 2^14)
//     w'.x' ~= wh.xh + wh.xl + wl.xh                                          (wl.xl ~ 2^-22 dropped)
// three fp16 MFMAs into ONE fp32 accumulator reproduce the fp32 product to ~2^-21 relative —
// the same order as the fp32 accumulation error itself and far inside the 1e-3 parity gate —
// at 3/16 of the cost.  The epilogue multiplies by 2^-(k+s) (ConvArgs::out_scale), exactly.
//
// Same contract and fusion as conv_mfma_f32.hip (A = packed weights, rows = cout; B = input
// pixels; GroupNorm-apply(+SiLU) prologue, virtual torch.cat, bias / time-embedding / residual
// epilogue) plus per-channel partial sums of the OUTPUT for the next GroupNorm.
//
// Data movement (what the fp16 rate makes necessary):
//   * every global->LDS transfer in the K loop is LDS-DMA (global_load_lds_dwordx4): no VGPRs
//     in flight, exact per-wave instruction counts, so counted s_waitcnt vmcnt(N) + raw
//     s_barrier keep two weight steps and the next activation chunk in flight across barriers;
//   * WEIGHTS go through a 3-slot LDS ring shared by all waves of the workgroup (one L2 read
//     per workgroup and step instead of one per wave: the per-wave register path was L2-bound);
//   * ACTIVATIONS of the next 32-channel chunk land raw (fp32) in LDS; each thread transforms
//     the slots it fetched itself (norm, SiLU, 2^s prescale, hi/lo split) into the MFMA image
//     [block 0/1][hi|lo][halo pixel][16 fp16] (32 B per pixel and plane: a fragment read is
//     2 x 512 contiguous bytes, conflict-free).
// K walk, wide chunks (CB = 2) and 1x1: 32 input channels (two 16-channel blocks) per step and tap; a trailing single
// block (Cin = 48, 144) pairs two TAPS per step instead.  16-channel chunks of a 3x3 (CB = 1, the default): two taps per
// step, and two chunks share the step that the ninth tap would leave half empty -- 4 + 5 steps per pair of chunks, the
// "pair walk" (conv_mfma_f16x3_body.h; conv16_num_steps in midd_internal.h is the one place that counts the steps).
#include "f16x3_common.h"
#include <cstdlib>
#include <type_traits>
#ifdef MIDD_CONV_TIMING
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>
#endif

namespace midd {

#ifndef MIDD_LDS_TARGET_KB
#define MIDD_LDS_TARGET_KB 52
#endif
#ifndef MIDD_RING_MAX
#define MIDD_RING_MAX 6
#endif
#ifndef MIDD_LDS_WIDE_KB
#define MIDD_LDS_WIDE_KB 78
#endif
// Geometry of one tile of this kernel, written down once as plain integers: Conv16Tile{ks, stride, tw, mt, nt, wm, wn, cbt} derives
// everything else.  Conv16Geom<> hands it to the kernel as constants; the tile picker and conv16_launch_info evaluate it at run time.
struct Conv16Tile {
    int ks, stride, tw, mt, nt, wm, wn;
    int cbt = 0;                                             // 16-channel blocks per chunk: 0 = conv16_cb(ks), 2 = the "wide" 3x3 variant
    int pl = 2;                                              // fp16 planes per operand: 2 = hi | lo (f16x3), 1 = the rounded value alone (compute "f16")
    int nw = wm * wn;
    int nthreads = nw * 64;
    int th = wm * mt * 16 / tw;
    int ih = (th - 1) * stride + ks;
    int iw = (tw - 1) * stride + ks;
    int npix = ih * iw;
    int cb = cbt ? cbt : conv16_cb(ks);
    int qpp = 4 * cb;                                        // 16-byte slots per halo pixel and chunk
    int nslot = npix * qpp;
    int apw = (nslot + nthreads - 1) / nthreads;             // activation DMA pieces per wave and chunk
    int raw_bytes = apw * nthreads * 16;
    int plane = npix * 32;
    int img_bytes = pl * cb * plane;
    int wpieces = wn * nt * pl;                              // 1 KiB weight pieces per step
    int ppw = (wpieces + nw - 1) / nw;                       // pieces per wave and step (duplicates pad)
    int wslice = wpieces * 1024;
    // epilogue state kept in LDS instead of registers (the K loop is register-bound): GroupNorm partial
    // sums of the output, one row [2][NT*16] per wave, and the bias (+ time embedding) vector of the workgroup
    int stat_floats = nw * 2 * nt * 16;
    int add_floats = wn * nt * 16;
    // GroupNorm scale/shift of the input, [2][Cin] floats, sized at launch (dynamic LDS); the ring is
    // dimensioned for up to NOMINAL_CIN input channels (more still runs, possibly one workgroup per CU fewer)
    static constexpr int NOMINAL_CIN = 384;
    int fixed_bytes = raw_bytes + img_bytes + (stat_floats + add_floats) * 4 + 2 * NOMINAL_CIN * 4 + 64;
    // weight steps resident in LDS (prefetch distance RING-1): L2->LDS latency is ~1-2k cycles under
    // load, a step is only 150-600 MFMA cycles, so take as many slots as fit in the LDS target, between 2 and MIDD_RING_MAX.
    // 52 KB: three workgroups per CU
    // (stride-2 tiles stage a 33x17 halo and run one workgroup per CU whatever the ring: they take a deep ring -- with two
    // slots the counted wait for a step's weights was 18-33 % of a wave's time, in-kernel stamps of round 3)
    // wide 3x3 chunks (launches that leave at most ~2 workgroups per CU anyway): two workgroups per CU
    int lds_target = (stride == 2 ? 120 : (ks == 3 && cb == 2) ? MIDD_LDS_WIDE_KB : MIDD_LDS_TARGET_KB) * 1024;
    int ring_fit = (lds_target - fixed_bytes) / wslice;
    int ring = ring_fit < 2 ? 2 : (ring_fit > MIDD_RING_MAX ? MIDD_RING_MAX : ring_fit);
    int lds_nominal = fixed_bytes + ring * wslice;           // at NOMINAL_CIN
    bool fits = lds_nominal <= 160 * 1024 && (ring - 2) * ppw + apw <= 60;      // LDS of a CU; the vmcnt encoding.  Else never picked, never instantiated
    constexpr int lds_bytes(int cin) const { return lds_nominal + 2 * (cin - NOMINAL_CIN) * 4; }   // incl. the 16 mean/rstd floats
};

template <int KS, int STRIDE, int TW, int MT, int NT, int WM, int WN, int CBT = 0, int PL = 2>
struct Conv16Geom {
    static constexpr Conv16Tile g{KS, STRIDE, TW, MT, NT, WM, WN, CBT, PL};
    static constexpr int NW = g.nw, NTHREADS = g.nthreads, TH = g.th, IH = g.ih, IW = g.iw, CB = g.cb, QPP = g.qpp, NSLOT = g.nslot, APW = g.apw;
    static constexpr int RAW_BYTES = g.raw_bytes, PLANE = g.plane, IMG_BYTES = g.img_bytes, WPIECES = g.wpieces, PPW = g.ppw, WSLICE = g.wslice;
    static constexpr int STAT_FLOATS = g.stat_floats, ADD_FLOATS = g.add_floats, RING = g.ring;
    static_assert((WM * MT * 16) % TW == 0, "tile");
};

// Diagnostic build only (-DMIDD_CONV_TIMING, tools/conv_timing.py): s_memtime stamps of wave 0 of every
// workgroup, summed per launch shape.  Shares, not run times: the stamps drain the LDS queue.
#ifdef MIDD_CONV_TIMING
enum { TS_WAIT, TS_ISSUE, TS_MFMA, TS_CHUNK_WAIT, TS_TRANSFORM, TS_EPILOGUE, TS_PROLOGUE, TS_FIRSTWAIT, TS_DMAWAIT, TS_RES, TS_PUBLISH, TS_TOTAL, TS_REAL, TS_WGS, TS_N };
__device__ unsigned long long g_conv_timing[64][TS_N];
__device__ __forceinline__ unsigned long long ts_stamp() {
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#define TS_DECL bool ts_after_epi = false; unsigned long long ts_acc[TS_N] = {}; unsigned long long ts_last = ts_stamp(); const unsigned long long ts_t0 = ts_last; const unsigned long long ts_r0 = __builtin_amdgcn_s_memrealtime();
#define TS(k) { const unsigned long long t_ = ts_stamp(); ts_acc[k] += t_ - ts_last; ts_last = t_; }
#else
#define TS_DECL
#define TS(k)
#endif

#ifndef MIDD_CONV16_WAVES_PER_SIMD
#define MIDD_CONV16_WAVES_PER_SIMD 3
#endif
// the register budget is capped so that as many workgroups as the LDS target allows are resident
// (2 -> 3 workgroups per CU is worth ~25 %: the phases of one workgroup do not overlap themselves)
// (stride-2 tiles stage a 33x17 halo: their LDS allows one workgroup per CU anyway, so they get the whole register file)
// (wide chunks: two workgroups per CU by their LDS, so two waves per SIMD's worth of registers)
// The 128-pixel tile with the folded res_conv needs ~200 registers: capped at 168 it spilled 51 of them at every tile boundary --
// 34 MB of scratch writes and as many reads per 256x256 launch (WRITE_SIZE 84 MB for a 50 MB output, tools/traffic_per_op.sh).
// With two waves per SIMD's worth of registers nothing spills: same-box +4.4 % split, +0.6 % unsplit (round 3).
#ifndef MIDD_RES_MT2_WAVES
#define MIDD_RES_MT2_WAVES 2
#endif
#define MIDD_CONV16_BOUNDS __launch_bounds__(WM * WN * 64, (WM * WN == 4 && STRIDE == 1) ? (CBT == 2 ? 2 : (RES && MT == 2) ? MIDD_RES_MT2_WAVES : MIDD_CONV16_WAVES_PER_SIMD) : 1)
// The kernel, compiled twice from one text (conv_mfma_f16x3_body.h says why): two planes / three products, one plane / one product
#define MIDD_CONV16_KERNEL conv_mfma_f16x3_kernel
#define MIDD_CONV16_PL 2
#include "conv_mfma_f16x3_body.h"
#undef MIDD_CONV16_KERNEL
#undef MIDD_CONV16_PL
#define MIDD_CONV16_KERNEL conv_mfma_f16_kernel
#define MIDD_CONV16_PL 1
#include "conv_mfma_f16x3_body.h"
#undef MIDD_CONV16_KERNEL
#undef MIDD_CONV16_PL

// ------------------------------------------------------------------------------ dispatch
#ifdef MIDD_CONV_TIMING
static std::vector<std::string> g_timing_names;
static int conv_timing_slot(int ks, int st, int tw, int mt, int nt, int wm, int wn, int oh, int cin, int cout, int B, int ring, int wgs) {
    char buf[160];
    snprintf(buf, sizeof buf, "k%d s%d tile(%d,%d,%d,%d,%d) ring%d out%d^2 %d->%d B%d wgs%d", ks, st, tw, mt, nt, wm, wn, ring, oh, cin, cout, B, wgs);
    for (size_t i = 0; i < g_timing_names.size(); ++i) if (g_timing_names[i] == buf) return (int)i;
    if (g_timing_names.size() >= 63) return 63;
    g_timing_names.push_back(buf);
    return (int)g_timing_names.size() - 1;
}
extern "C" __attribute__((visibility("default"))) void mi_debug_conv_timing_dump(void) {
    static unsigned long long h[64][TS_N];
    (void)hipDeviceSynchronize();
    (void)hipMemcpyFromSymbol(h, HIP_SYMBOL(g_conv_timing), sizeof h);
    static const char* names[] = {"barrier", "dma-issue", "frag+mfma", "chunk-wait", "transform", "epilogue", "prologue", "wait-after-epi", "dma-wait", "res-phase", "publish"};
    for (size_t i = 0; i < g_timing_names.size(); ++i) {
        const double tot = (double)h[i][TS_TOTAL], wgs = (double)h[i][TS_WGS];
        if (wgs == 0) continue;
        printf("%-70s cyc/wg %9.0f clk %.2f GHz |", g_timing_names[i].c_str(), tot / wgs, tot / (double)h[i][TS_REAL] * 0.1);
        for (int k = 0; k < 11; ++k) printf(" %s %4.1f%%", names[k], 100.0 * (double)h[i][k] / tot);
        printf("\n");
    }
    memset(h, 0, sizeof h);
    (void)hipMemcpyToSymbol(HIP_SYMBOL(g_conv_timing), h, sizeof h);
    fflush(stdout);
}
#endif
template <int KS, int STRIDE, int TW, int MT, int NT, int WM, int WN, bool RES, int CBT = 0, int PL = 2>
static hipError_t launch16(const ConvArgs& a0, hipStream_t s) {
    using G = Conv16Geom<KS, STRIDE, TW, MT, NT, WM, WN, CBT, PL>;
    ConvArgs a = a0;
    a.tiles_x = (a.OW + TW - 1) / TW;
    a.tiles_y = (a.OH + G::TH - 1) / G::TH;
    const int ny = a.Cout / (WN * NT * 16);
    a.wgs_per_img = conv16_wgs_per_img(a.tiles_x * a.tiles_y, a.B, ny, a.persist_wgs);
    dim3 grid(a.B * a.wgs_per_img, ny);
#ifdef MIDD_CONV_TIMING
    a.dbg_slot = conv_timing_slot(KS, STRIDE, TW, MT * 10 + G::CB, NT, WM, WN, a.OH, a.C0 + a.C1, a.Cout, a.B, G::RING, (int)grid.x * (int)grid.y);
#endif
    if constexpr (G::g.fits) {
        const int lds_bytes = G::g.lds_bytes(a.C0 + a.C1);
        if (lds_bytes > 160 * 1024) return hipErrorInvalidValue;
        {
            static int raised[MIDD_MAX_DEVICES] = {};      // per instantiation and device
            hipError_t e = ensure_dynamic_lds(PL == 2 ? reinterpret_cast<const void*>(&conv_mfma_f16x3_kernel<KS, STRIDE, TW, MT, NT, WM, WN, RES, CBT>)
                                                      : reinterpret_cast<const void*>(&conv_mfma_f16_kernel<KS, STRIDE, TW, MT, NT, WM, WN, RES, CBT>), lds_bytes, raised);
            if (e != hipSuccess) return e;
        }
        if ((double)a.H * a.W * 64.0 >= 4294967296.0) return hipErrorInvalidValue;  // 32-bit DMA offsets inside one block plane
        if constexpr (PL == 2) hipLaunchKernelGGL((conv_mfma_f16x3_kernel<KS, STRIDE, TW, MT, NT, WM, WN, RES, CBT>), grid, dim3(G::NTHREADS), lds_bytes, s, a);
        else hipLaunchKernelGGL((conv_mfma_f16_kernel<KS, STRIDE, TW, MT, NT, WM, WN, RES, CBT>), grid, dim3(G::NTHREADS), lds_bytes, s, a);
        return hipGetLastError();
    } else {
        return hipErrorInvalidValue;        // tile never picked (conv16_pick_tile), not instantiated
    }
}

// ~3 resident workgroups per CU; a sample's tiles are dealt evenly to its persistent workgroups
int conv16_wgs_per_img(int tiles, int B, int ny, int target) {
    const int target_wgs = target ? target : 768;
    int per_img = target_wgs / (B * ny);
    if (per_img < 1) per_img = 1;
    if (per_img > tiles) per_img = tiles;
    const int tiles_per_wg = (tiles + per_img - 1) / per_img;
    return (tiles + tiles_per_wg - 1) / tiles_per_wg;
}

// Tiles the picker can reach.  Measured and dropped (same-box A/B at B=8, 256x256, round 1 and again in round 2 on the
// atomics-statistics build): 16x16-pixel tiles (MT = 4: -2..-3 %), 96-cout tiles (NT = 6: -1.7 %), 4x2-wave and 8-wave
// workgroups (neutral to negative).
#define MIDD_CONV16_TILES(X)                  \
    /*  tw  mt nt wm wn */                    \
    X(16, 2, 3, 4, 1) X(16, 1, 3, 4, 1) X(8, 1, 3, 2, 1) \
    X(16, 2, 3, 2, 2) X(16, 1, 3, 2, 2) X(8, 1, 3, 1, 2) \
    X(16, 2, 3, 1, 3) X(8, 1, 3, 1, 3)                   \
    X(16, 2, 3, 1, 4) X(8, 2, 3, 1, 4) X(8, 1, 3, 1, 4)  \
    X(16, 2, 2, 4, 1) X(8, 1, 2, 2, 1)                   \
    X(16, 2, 2, 2, 2) X(8, 1, 2, 1, 2)                   \
    X(16, 2, 1, 4, 1) X(8, 1, 1, 2, 1)

struct Tile16 { int tw, mt, nt, wm, wn; };
static const Tile16 kTiles16[] = {
#define X(tw, mt, nt, wm, wn) {tw, mt, nt, wm, wn},
    MIDD_CONV16_TILES(X)
#undef X
};

// the kernel's constants are the run-time geometry, for every listed tile at the three kernel shapes
#define X(tw, mt, nt, wm, wn)                                                                                     \
    static_assert(Conv16Geom<3, 1, tw, mt, nt, wm, wn>::RING == Conv16Tile{3, 1, tw, mt, nt, wm, wn}.ring &&         \
                  Conv16Geom<3, 2, tw, mt, nt, wm, wn>::APW == Conv16Tile{3, 2, tw, mt, nt, wm, wn}.apw &&           \
                  Conv16Geom<1, 1, tw, mt, nt, wm, wn>::WSLICE == Conv16Tile{1, 1, tw, mt, nt, wm, wn}.wslice, "Conv16Geom");
MIDD_CONV16_TILES(X)
#undef X
// ... and with one plane (compute "f16"): the same tile table, instantiated with PL = 1.  Halved weight slices and image: the
// LDS target buys a deeper ring (e.g. the 2x2-wave 96-cout tile: 6 KB slices, five slots instead of two)
#define X(tw, mt, nt, wm, wn)                                                                                                 \
    static_assert(Conv16Geom<3, 1, tw, mt, nt, wm, wn, 0, 1>::RING == Conv16Tile{3, 1, tw, mt, nt, wm, wn, 0, 1}.ring &&         \
                  Conv16Geom<3, 2, tw, mt, nt, wm, wn, 0, 1>::APW == Conv16Tile{3, 2, tw, mt, nt, wm, wn, 0, 1}.apw &&           \
                  Conv16Geom<1, 1, tw, mt, nt, wm, wn, 0, 1>::WSLICE * 2 == Conv16Tile{1, 1, tw, mt, nt, wm, wn}.wslice, "Conv16Geom, one plane");
MIDD_CONV16_TILES(X)
#undef X

// the 4x1-wave 3x3 tiles (mt = 1, 2) have a wide-chunk variant
static bool wide16_tile(const ConvTile& t) { return t.ks == 3 && t.stride == 1 && t.tw == 16 && t.nt == 3 && t.wm == 4 && t.wn == 1; }
// Launches whose grid is at most this many workgroups take the wide-chunk variant of the 4x1-wave tiles (they would
// leave the third workgroup slot of a CU empty anyway).
#ifndef MIDD_WIDE_MAX_WGS
#define MIDD_WIDE_MAX_WGS 512
#endif
bool conv16_pick_tile(int Cin, int Cout, int B, int OH, int OW, int ks, int stride, ConvTile* t, bool allow_wide, int planes) {
    if (Cout % 16) return false;
    if (!((ks == 3 && (stride == 1 || stride == 2)) || (ks == 1 && stride == 1))) return false;
    if (ks == 1 && conv1x1_pick_tile(Cin, Cout, B, OH, OW, t)) { t->pl = planes; return true; }      // dedicated 1x1 kernel (conv1x1_f16x3.hip)
    const int nt = (Cout % 48 == 0) ? 3 : (Cout % 32 == 0) ? 2 : 1;
    const Tile16* best = nullptr;
    long best_score = -(1L << 60), best_wgs = 0;
    // 192, not 256 workgroups: at B=4 (half-batches) the 32x32 layers with 144 couts would otherwise drop to 32-pixel
    // 2-wave tiles that stream the weights twice as often (same-box A/B: +1.7 %)
    constexpr long min_wgs = 192;
    for (const Tile16& d : kTiles16) {
        if (d.nt != nt) continue;
        const int nn_d = Cout / (16 * d.nt);              // cout slices of 16*nt; a workgroup takes wn of them
        if (nn_d % d.wn) continue;
        if (!Conv16Tile{ks, stride, d.tw, d.mt, d.nt, d.wm, d.wn, 0, planes}.fits) continue;
        const int bm = d.wm * d.mt * 16, th = bm / d.tw;
        const long tiles = (long)((OW + d.tw - 1) / d.tw) * ((OH + th - 1) / th);
        const long wgs = (long)B * tiles * (nn_d / d.wn);
        const long covered = tiles * d.tw * th;
        const bool wasteful = covered * 4 > (long)OH * OW * 5;
        // enough workgroups first; then the pixels one weight fetch is shared over (the weight stream from L2 is what
        // starves small tiles), then the couts one activation staging is shared over
        const long share = (long)bm * 8 + d.wn;
        // (forcing the 2x2-wave 96-cout tile on the <= 32x32 / <= 64x64 maps -- the GroupNorm / SiLU / split transform shared by
        // two cout slices -- measured -6.5 % / -7 %: its 12 KB weight slices leave a two-slot ring, one step in flight)
        const long score = (wgs >= min_wgs ? 1000000 : wgs * (1000000 / min_wgs)) + share - (wasteful ? 500000 : 0);
        if (score > best_score) { best_score = score; best = &d; best_wgs = wgs; }
    }
    if (!best) return false;
    // compute "f16" (planes == 1) keeps these choices: the score does not look at the planes (which tiles the halved slices
    // would newly favour is unmeasured: DESIGN.md section 4)
    *t = ConvTile{ks, stride, best->tw, best->mt, best->nt, best->wm, best->wn, 0, planes};
    if (allow_wide && wide16_tile(*t) && Cin >= 32 &&
        best_wgs <= MIDD_WIDE_MAX_WGS && Conv16Tile{ks, stride, best->tw, best->mt, best->nt, best->wm, best->wn, 2, planes}.fits)
        t->cb = 2;
    return true;
}

bool conv16_launch_info(int Cin, int Cout, int B, int OH, int OW, const ConvTile& t, int persist_wgs, ConvLaunchInfo* o) {
    if (t.ks == 1 && t.tw == 0) return conv1x1_launch_info(Cin, Cout, B, OH, OW, t, persist_wgs, ATT_NONE, o);
    // only what conv16_launch instantiates: a listed tile at 3x3 s1 / 3x3 s2 / 1x1, or one of the two wide tiles
    bool listed = false;
    if (t.cb == 2 ? wide16_tile(t) : ((t.ks == 3 && (t.stride == 1 || t.stride == 2)) || (t.ks == 1 && t.stride == 1)))
        for (const Tile16& d : kTiles16) listed = listed || (d.tw == t.tw && d.mt == t.mt && d.nt == t.nt && d.wm == t.wm && d.wn == t.wn);
    if (!listed) return false;
    if (t.pl != 1 && t.pl != 2) return false;
    const Conv16Tile g{t.ks, t.stride, t.tw, t.mt, t.nt, t.wm, t.wn, t.cb == 2 ? 2 : 0, t.pl};
    o->tiles_x = (OW + t.tw - 1) / t.tw; o->tiles_y = (OH + g.th - 1) / g.th;
    o->grid_y = Cout / (t.wn * t.nt * 16);
    o->wgs_per_img = conv16_wgs_per_img(o->tiles_x * o->tiles_y, B, o->grid_y, persist_wgs);
    o->grid_x = B * o->wgs_per_img;
    o->ring = g.ring; o->ppw = g.ppw; o->apw = g.apw; o->lds_bytes = g.lds_bytes(Cin);
    return true;
}

// the dispatch of one arithmetic mode: PL fp16 planes per operand
template <int PL>
static hipError_t conv16_dispatch(const ConvArgs& a, const ConvTile& t, hipStream_t s) {
    if (t.cb == 2) {          // wide chunks: the two 4x1-wave tiles the picker marks (conv16_pick_tile)
        if (!wide16_tile(t)) return hipErrorInvalidValue;
        if (t.mt == 2) return a.res_steps > 0 ? launch16<3, 1, 16, 2, 3, 4, 1, true, 2, PL>(a, s) : launch16<3, 1, 16, 2, 3, 4, 1, false, 2, PL>(a, s);
        if (t.mt == 1) return a.res_steps > 0 ? launch16<3, 1, 16, 1, 3, 4, 1, true, 2, PL>(a, s) : launch16<3, 1, 16, 1, 3, 4, 1, false, 2, PL>(a, s);
        return hipErrorInvalidValue;
    }
#define X(tw_, mt_, nt_, wm_, wn_)                                                            \
    if (t.tw == tw_ && t.mt == mt_ && t.nt == nt_ && t.wm == wm_ && t.wn == wn_) {           \
        if (t.ks == 3 && t.stride == 1 && a.res_steps > 0) return launch16<3, 1, tw_, mt_, nt_, wm_, wn_, true, 0, PL>(a, s); \
        if (t.ks == 3 && t.stride == 1) return launch16<3, 1, tw_, mt_, nt_, wm_, wn_, false, 0, PL>(a, s); \
        if (t.ks == 3 && t.stride == 2) return launch16<3, 2, tw_, mt_, nt_, wm_, wn_, false, 0, PL>(a, s); \
        if (t.ks == 1 && t.stride == 1) return launch16<1, 1, tw_, mt_, nt_, wm_, wn_, false, 0, PL>(a, s); \
    }
    MIDD_CONV16_TILES(X)
#undef X
    return hipErrorInvalidValue;
}

hipError_t conv16_launch(const ConvArgs& a, const ConvTile& t, hipStream_t s) {
    if (t.ks == 1 && t.tw == 0) return conv1x1_launch(a, t, s);
    if (t.pl == 2) return conv16_dispatch<2>(a, t, s);
    if (t.pl == 1) return conv16_dispatch<1>(a, t, s);
    return hipErrorInvalidValue;
}

}  // namespace midd
