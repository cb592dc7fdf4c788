// The body of the fp16-MFMA implicit-GEMM convolution kernel (conv_mfma_f16x3.hip: number format, data movement and DMA
// protocol are described there).  Not a header in the usual sense: conv_mfma_f16x3.hip includes this text TWICE, with
//   MIDD_CONV16_KERNEL = conv_mfma_f16x3_kernel, MIDD_CONV16_PL = 2   two fp16 planes per operand (hi | lo), three MFMAs per product
//   MIDD_CONV16_KERNEL = conv_mfma_f16_kernel,   MIDD_CONV16_PL = 1   compute "f16": one plane (the same prescaled value rounded
//                                                                    once, no lo half) in the staged image and the weight slices,
//                                                                    one MFMA per product
// Everything else (DMA protocol, prologue, epilogue, statistics) is the same code; the geometry and every counted wait follow
// from Conv16Tile::pl.  Why textual: a shared __device__ body inlined into two entry points made the compiler allocate
// registers differently (one split-fp16 instantiation began to spill 36 registers), and a further template parameter would
// rename the split-fp16 symbols that profiles and the plan dump name.  Compiled this way the split-fp16 kernels' ISA is,
// instruction for instruction, what it was before the one-plane kernels existed.
#if !defined(MIDD_CONV16_KERNEL) || !defined(MIDD_CONV16_PL)
#error "include from conv_mfma_f16x3.hip with MIDD_CONV16_KERNEL and MIDD_CONV16_PL defined"
#endif

template <int KS, int STRIDE, int TW, int MT, int NT, int WM, int WN, bool RES, int CBT>
__global__ MIDD_CONV16_BOUNDS void MIDD_CONV16_KERNEL(const ConvArgs a) {
    constexpr int PL = MIDD_CONV16_PL;
    static_assert(PL == 1 || PL == 2, "planes");
    using G = Conv16Geom<KS, STRIDE, TW, MT, NT, WM, WN, CBT, PL>;
    constexpr int NW = G::NW, NTHREADS = G::NTHREADS, TH = G::TH, IW = G::IW;
    constexpr int PAD = (KS == 3) ? 1 : 0;
    constexpr int NSLOT = G::NSLOT, APW = G::APW, PLANE = G::PLANE;
    constexpr int TAPS = KS * KS;
    constexpr int HSTEPS = (TAPS + 1) / 2;
    constexpr int PPW = G::PPW, WSLICE = G::WSLICE, RING = G::RING;

    extern __shared__ __attribute__((aligned(16))) char lds[];             // G::lds_bytes(Cin)
    char* const raw = lds;
    char* const img = lds + G::RAW_BYTES;
    char* const wring = img + G::IMG_BYTES;
    float* const stat_lds = reinterpret_cast<float*>(wring + RING * WSLICE);   // [wave][2][NT*16]
    float* const add_lds = stat_lds + G::STAT_FLOATS;                           // [WN*NT*16]
    float* const gnp = add_lds + G::ADD_FLOATS;                                 // [2][Cin] scale, shift

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wn = wave % WN;
    const int wm = wave / WN;
    const int p16 = lane & 15;
    const int kq = lane >> 4;

    // Persistent workgroups: blockIdx.x = (sample, j); the workgroup walks tiles j, j+wgs_per_img, ...
    // of ITS sample, so the weight ring streams cyclically across tiles and the next tile's first
    // activation chunk is already in flight while this tile is finished and stored.
    const int tiles_per_img = a.tiles_x * a.tiles_y;
    const int b = blockIdx.x / a.wgs_per_img;
    int trem = blockIdx.x - b * a.wgs_per_img;            // current tile of this sample
    int oy0 = (trem / a.tiles_x) * TH, ox0 = (trem % a.tiles_x) * TW;

    const int Cin = a.C0 + a.C1;
    const int nblk = Cin >> 4;
    constexpr int CB = G::CB, QPP = G::QPP;
    const int nchunks = (nblk + CB - 1) / CB;
    const int ntiles_total = a.Cout >> 4;
    const int ntile_wg = blockIdx.y * (WN * NT);          // first cout tile of this workgroup
    const int res_steps = RES ? a.res_steps : 0;          // folded res_conv: K steps after a tile's 3x3 steps (instantiations of their own: registers)
    const int total_steps = conv16_num_steps(Cin, TAPS, G::CB) + res_steps;

    // ---- weights: LDS-DMA ring ---------------------------------------------------------------
    // global layout [step][cout tile][hi|lo (PL planes)][lane] x 16 B; the workgroup's slice of one step is
    // contiguous.  Everything but the lane offset is wave-uniform, so the address arithmetic stays
    // on the scalar unit.
    constexpr int WTILE = PL * 1024;                      // bytes of one cout tile's planes in a step
    const char* const wbase = reinterpret_cast<const char*>(a.wpack) + (size_t)ntile_wg * WTILE;
    const size_t wstep_bytes = (size_t)ntiles_total * WTILE;
    const int lane16 = lane * 16;
    int wr_step = 0, wr_slot = 0;                         // next step to fetch / the ring slot it goes to
    const char* wr_src = wbase;                           // = wbase + wr_step * wstep_bytes, kept incrementally
    // Diagnostic build (-DMIDD_DMA_CHECK, tools/dma_check.sh; never shipped): every destination of an asynchronous transfer -- ring
    // slot pieces, landing-buffer slots, the registers of untracked loads -- is filled with a NaN sentinel before the transfer is
    // requested, and every consumer checks what it reads: a counted wait that returns before its data has landed leaves the
    // sentinel in place and sets STATUS_DMA_EARLY.  Run over the whole GPU suite this checks the hand-counted vmcnt protocol
    // on the hardware, for every instantiation and schedule the tests reach.
#ifdef MIDD_DMA_CHECK
    constexpr unsigned SENT_W = 0x7FFF7FFFu;              // two fp16 NaNs: no packed weight
    constexpr unsigned SENT_A = 0x7FC0DEADu;              // an fp32 NaN: no finite activation
    unsigned dma_bad = 0;
    auto sent4 = [](unsigned v) { typedef unsigned u32x4_ __attribute__((ext_vector_type(4))); return __builtin_bit_cast(f32x4, (u32x4_){v, v, v, v}); };
    auto has_sent = [](const auto& q, unsigned v) {
        typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
        const u32x4_ u = __builtin_bit_cast(u32x4_, q);
        return (unsigned)((u[0] == v) | (u[1] == v) | (u[2] == v) | (u[3] == v));
    };
#endif
    auto issue_w = [&]() {
        char* slot = wring + wr_slot * WSLICE;
#ifdef MIDD_DMA_CHECK
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            int piece = (WM == 1) ? wave * PPW + i : wave + i * NW;
            if (piece >= G::WPIECES) piece -= G::WPIECES;
            if constexpr (PL == 1) piece %= G::WPIECES;
            lds_store_raw(slot + piece * 1024 + lane16, sent4(SENT_W));
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
#pragma unroll
        for (int i = 0; i < PPW; ++i) {
            // WM == 1: every wave owns a distinct cout slice, so it fetches exactly the pieces it
            // reads itself (no cross-wave hand-off, no barrier per step); otherwise round-robin.
            int piece = (WM == 1) ? wave * PPW + i : wave + i * NW;
            if (piece >= G::WPIECES) piece -= G::WPIECES;          // padding duplicate: same bytes, same place (issuing only the
                                                                   // WPIECES distinct pieces, with per-wave wait counts, measured -1 %: round 3)
            if constexpr (PL == 1) piece %= G::WPIECES;            // one plane, 16 couts, four waves: ONE piece per step, three duplicates
            dma16(wr_src + piece * 1024 + lane16, slot + piece * 1024);
        }
        ++wr_step; wr_src += wstep_bytes;
        if (wr_step == total_steps) { wr_step = 0; wr_src = wbase; }   // cyclic: step 0 of the next tile follows the last
        wr_slot = (wr_slot + 1 == RING) ? 0 : wr_slot + 1;
    };

    // ---- activations: per-thread slots (halo pixel, 4-channel quad q8 of the 32-channel chunk) ----
    const int q8 = tid % QPP;                             // (NTHREADS % QPP == 0: constant per thread)
    const int sblk = q8 >> 2;
    int g_off[APW];            // pixel index inside the sample's image; -1: out of the image; -2: slot beyond the tile
    bool tile_pad = true;      // (uniform) the tile's halo leaves the image somewhere: only then a slot can be out of the image
    auto set_tile = [&](int t) {
        const int iy0 = (t / a.tiles_x) * TH * STRIDE - PAD, ix0 = (t % a.tiles_x) * TW * STRIDE - PAD;
        tile_pad = iy0 < 0 || ix0 < 0 || iy0 + G::IH > a.H || ix0 + IW > a.W;
        // opaque copy of the thread index: a slot's halo row / column is worked out HERE, once per tile (a handful of
        // instructions), instead of being hoisted into 2 * APW registers that stay live across the whole K loop
        int tid_ = tid;
        asm volatile("" : "+v"(tid_));
#pragma unroll
        for (int s = 0; s < APW; ++s) {
            const int slot = tid_ + s * NTHREADS;
            int off = -2;
            if (slot < NSLOT) {
                const int pix = slot / QPP;
                const int iy = pix / IW, ix = pix - iy * IW;
                const int gy = iy0 + iy, gx = ix0 + ix;
                off = (gy >= 0 && gy < a.H && gx >= 0 && gx < a.W) ? gy * a.W + gx : -1;
            }
            g_off[s] = off;
        }
    };
    set_tile(trem);
    // Lanes with nothing to fetch (padding, unused slots, missing second block) read a valid
    // dummy address; transform() writes zeros / nothing for them.
    auto issue_a = [&](int c) {
        // channel-blocked activations [B][C/16][H][W][16]: the chunk's 16-channel block of a halo row is one contiguous run
        const int blk = min(CB * c + sblk, nblk - 1);
        const float* src; int bsrc, nb;
        if ((blk << 4) < a.C0) { src = a.src0; bsrc = blk; nb = a.C0 >> 4; }
        else                   { src = a.src1; bsrc = blk - (a.C0 >> 4); nb = a.C1 >> 4; }
        const char* base = reinterpret_cast<const char*>(src) + ((size_t)(b * nb + bsrc) * (size_t)(a.H * a.W)) * 64 + (q8 & 3) * 16;
#ifdef MIDD_DMA_CHECK
#pragma unroll
        for (int s = 0; s < APW; ++s) lds_store_raw(raw + (wave + s * NW) * 1024 + lane16, sent4(SENT_A));
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#endif
#pragma unroll
        for (int s = 0; s < APW; ++s) {
            const unsigned byte_off = (unsigned)max(g_off[s], 0) * 64u;             // one block plane is < 4 GiB (host-checked)
            dma16(base + byte_off, raw + (wave + s * NW) * 1024);
        }
    };
    // The transform of a chunk, per slot: read the raw fp32 quad, GroupNorm-apply (+SiLU), 2^s prescale, hi/lo split,
    // write into the MFMA image.  (Measured in round 2: running the arithmetic of chunk c+1's transform under the MFMAs
    // of chunk c's steps 2..4 and only the LDS writes at the chunk boundary is 2-4 % SLOWER end to end -- the waves
    // reach the step barriers out of phase.)
    float rscale = RAW_PRESCALE;          // 2^a of a raw operand (set after the prologue's barrier)
    // The transform of a chunk, per slot: raw fp32 quad -> GroupNorm-apply (+SiLU) -> 2^s prescale -> hi/lo split -> MFMA image.
    // Instruction diet of round 3 (the vector ALU is what a chunk costs beside its MFMAs):
    //   * all raw quads of the chunk are requested before the first is used (one LDS round trip, not APW);
    //   * SiLU on the exponent's own argument: the prologue leaves sc' = -log2(e) rstd gamma, sh' = -log2(e) (beta - mean rstd gamma),
    //     so t = x sc' + sh' = -y log2(e) feeds v_exp directly, d = (1 + 2^t) / 16 is ONE fma, and the operand is
    //     u = t / d = -16 log2(e) silu(y); the constant -ln 2 that turns u back into 16 silu(y) sits in the packed
    //     weights (pack_conv_f16x3: SILU_WEIGHT_FACTOR) -- 5 instructions per element instead of 6, 2 of them transcendental;
    //   * hi = fp16(u) by v_cvt_pk_f16_f32, lo = fp16(u - hi) by ONE v_fma_mix per element (f16x3_common.h: split_pair);
    //   * no select for the conv's zero padding: out-of-image slots are zeroed ONCE per tile (first chunk) and otherwise
    //     simply not written (g_off < 0 also covers a thread's slot beyond the tile): the only conditional code is
    //     the pair of LDS stores.
    // (Measured in round 2: running the arithmetic of chunk c+1's transform under the MFMAs of chunk c's steps 2..4 and
    // only the LDS writes at the chunk boundary is 2-4 % SLOWER end to end -- the waves reach the step barriers out of phase.)
    auto transform = [&](int c) {
        const int blk = CB * c + sblk;
        if (blk >= nblk) return;
        const int ch = (blk << 4) + (q8 & 3) * 4;
        f32x4 rq[APW];
#pragma unroll
        for (int s = 0; s < APW; ++s) rq[s] = *reinterpret_cast<const f32x4*>(raw + (tid + s * NTHREADS) * 16);
#ifdef MIDD_DMA_CHECK
#pragma unroll
        for (int s = 0; s < APW; ++s) dma_bad |= has_sent(rq[s], SENT_A);
#endif
        f32x4 sc = {rscale, rscale, rscale, rscale}, sh = {0.f, 0.f, 0.f, 0.f};      // raw operand: per-sample 2^a (stats_common.h)
        if (a.prologue != PRO_RAW) {
            sc = *reinterpret_cast<const f32x4*>(gnp + ch);
            sh = *reinterpret_cast<const f32x4*>(gnp + Cin + ch);
        }
        char* base = img + sblk * PL * PLANE + (q8 & 3) * 8;
        typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
        if (c == 0 && tile_pad) {                  // (uniform) first chunk of a tile whose halo leaves the image: the conv's zero padding
#pragma unroll
            for (int s = 0; s < APW; ++s) {
                const int slot = tid + s * NTHREADS;
                if (g_off[s] == -1) {                  // (a thread's slots cover ITS 16-channel block: all blocks get zeroed between the threads)
                    *reinterpret_cast<u32x2*>(base + (slot / QPP) * 32) = (u32x2){0u, 0u};
                    if constexpr (PL == 2) *reinterpret_cast<u32x2*>(base + PLANE + (slot / QPP) * 32) = (u32x2){0u, 0u};
                }
            }
        }
#pragma unroll
        for (int s = 0; s < APW; ++s) {
            const int slot = tid + s * NTHREADS;
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __builtin_fmaf(rq[s][e], sc[e], sh[e]);
#if defined(C16_ABL) && C16_ABL == 4     // ablation 4 (wrong results): no SiLU
            if (false) {
#else
            if (a.prologue == PRO_GN_SILU) {
#endif
#pragma unroll
                for (int e = 0; e < 4; ++e) {      // v = t = -y log2(e):  u = t * 16 / (1 + 2^t)
                    const float d = __builtin_fmaf(__builtin_amdgcn_exp2f(v[e]), 1.0f / ACT_PRESCALE, 1.0f / ACT_PRESCALE);
                    v[e] = v[e] * __builtin_amdgcn_rcpf(d);
                }
            }
            unsigned h01, h23, l01, l23;
            planes_pair<PL>(v[0], v[1], h01, l01);
            planes_pair<PL>(v[2], v[3], h23, l23);
            if (g_off[s] >= 0) {                   // in the image and in the tile
                const int pix = slot / QPP;
                *reinterpret_cast<u32x2*>(base + pix * 32) = (u32x2){h01, h23};
                if constexpr (PL == 2) *reinterpret_cast<u32x2*>(base + PLANE + pix * 32) = (u32x2){l01, l23};
            }
        }
    };

    // ---- per-lane LDS byte offsets of the B fragments (tap (0,0), block 0, hi plane) ----
    int frag_base[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        const int pp = (wm * MT + mt) * 16 + p16;
        const int py = pp / TW, px = pp - py * TW;
        frag_base[mt] = ((py * STRIDE) * IW + px * STRIDE) * 32 + (kq & 1) * 16;
    }
    int frag_full[MT];                                    // full chunk: lanes kq>=2 read block 1
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) frag_full[mt] = frag_base[mt] + (kq >> 1) * PL * PLANE;
    const int wfrag_off = (wn * NT) * WTILE + lane * 16;  // this wave's cout tiles inside a ring slot

    f32x4 acc[MT][NT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt)
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};

    // ---- K loop -------------------------------------------------------------------------------
    // DMA protocol (D = RING-1 weight steps in flight).  Per wave, in program order:
    //   prologue : A(0) W(0)..W(D-1)                                   -> wait 0
    //   step s   : wait; barrier; issue W(s+D) [; issue A(c+1) in the first step of a chunk]; MFMAs
    //   chunk end: wait; barrier; transform(c+1)
    // When step s waits, the groups younger than W(s) are W(s+1..s+D-1), plus A(c+1) during steps
    // 1..D of the chunk (afterwards A(c+1) is older than W(s), i.e. already forced complete):
    //   N = (D-1)*PPW [+ APW].   At the chunk end the groups younger than A(c+1) are the
    // min(nsteps-1, D) weight groups issued after it.  The slot refilled after the barrier of step
    // s, (s+D)%RING == (s-1)%RING, was last read before that barrier by every wave.
    //
    // Pair walk (PAIR: 3x3, 16-channel chunks).  Chunks of a tile are taken in pairs (c even, c + 1): 4 steps, taps (0|1)
    // (2|3) (4|5) (6|7) of block c, then 5 steps, (tap 8 of block c | tap 0 of block c + 1), (1|2) (3|4) (5|6) (7|8) of block
    // c + 1; an unpaired last chunk keeps 5 steps with a zero-weight upper half.  One image buffer: after its fourth step the
    // even chunk reads its tap-8 fragments into xh / xl (dead until the next step), the chunk end's lgkmcnt(0) + barrier
    // retire them before transform(c + 1) rewrites the image, and the odd chunk's first step loads tap 0 of the new image
    // into lanes kq >= 2 only.  Per step nothing changes: none of the counts above depends on the chunk's length S
    // (step j of a chunk waits for W(s0+j); A(c+1) follows W(s0+D) in program order, so it is younger for 1 <= j <= D
    // whatever S is, and from the chunk end on it has landed).  What does depend on S is the chunk end: the groups younger
    // than A(c+1) are the S-1 weight groups of steps 1..S-1 plus those of the res steps (the res phase's own loads have all
    // been awaited inside it, and operations retire in order), `after` in all, of which at most D can still be outstanding:
    //   vmcnt(min(after, D) * PPW)     for EVERY after in 0..D -- S = 4 gives after = 3, which with a five- or six-slot
    // ring (D = 4, 5) is neither >= D nor 1: the former ladder (>= D, == 1, else 0) would have drained the ring there.
    constexpr int D = RING - 1;
    constexpr bool PAIR = conv16_pair_walk(TAPS, CB);
    static_assert(D <= 5, "the chunk-end wait has one arm per after = 1 .. 4 below D (MIDD_RING_MAX 6)");
    constexpr auto cmin = [](int x, int y) { return x < y ? x : y; };
    const int ntile0 = ntile_wg + wn * NT;
    TS_DECL
    issue_a(0);
#pragma unroll
    for (int i = 0; i < D; ++i) issue_w();
    // (Measured in round 2: requesting the totals BEFORE the DMAs through loads the compiler does not track, with a counted
    // wait, so that the GroupNorm arithmetic overlaps the DMA latency instead of following it -- 0 % split, -0.7 % unsplit.)
#if !(defined(C16_ABL) && C16_ABL == 6)  // ablation 6 (wrong results): no GroupNorm prologue
    if (a.prologue == PRO_GN || a.prologue == PRO_GN_SILU)       // GroupNorm scale / shift of this sample (stats_common.h)
        gn_prologue_lds(a.gn_tot0, a.C0, a.gn_bs0, a.gn_tot1, a.C1, a.gn_bs1, a.stat_rep, a.gn_gamma, a.gn_beta, a.gn_eps, a.gn_inv_n, b,
                        (a.prologue == PRO_GN_SILU) ? SILU_ARG_FACTOR : ACT_PRESCALE, gnp, tid, NTHREADS, a.status);
#endif
    // raw operand: its sum of squares from the producers' totals -> power-of-two prescale (stats_common.h); the scale /
    // shift area is free in this case
    stat_word* const raw_acc = reinterpret_cast<stat_word*>(gnp);
    if (a.prologue == PRO_RAW && a.gn_tot0 != nullptr && wave == 0)
        raw_sumsq_lds(a.gn_tot0, a.C0, a.gn_bs0, a.gn_tot1, a.C1, a.gn_bs1, a.stat_rep, b, raw_acc, lane);
    // folded res_conv: its operand is the (raw) block input; same prescale rule, from the block input's totals
    stat_word* const res_acc = reinterpret_cast<stat_word*>(gnp + 2 * Cin);          // the 64 spare bytes behind the scale / shift table
    if (res_steps > 0 && a.res_tot0 != nullptr && wave == NW - 1)
        raw_sumsq_lds(a.res_tot0, a.res_C0, a.res_bs0, a.res_tot1, a.res_C1, a.res_bs1, a.stat_rep, b, res_acc, lane);
    {
        const int trow = (a.temb != nullptr) ? a.trow[b] : 0;
        for (int i = tid; i < G::ADD_FLOATS; i += NTHREADS) {
            const int co = ntile_wg * 16 + i;
            add_lds[i] = a.bias[co] + (a.temb != nullptr ? a.temb[(size_t)trow * a.temb_stride + co] : 0.f);
        }
    }
    wait_vm_and_barrier<0>();               // everything above has landed / is visible (once per launch)
    float oscale = a.out_scale;             // epilogue factor: undoes the weight and the operand prescale (exact)
    if (a.prologue == PRO_RAW) {
        rscale = a.raw_scale_fixed;
        if (a.gn_tot0 != nullptr) {
            bool bad;
            const int ex = __builtin_amdgcn_readfirstlane(raw_prescale_exp(raw_acc, &bad));
            rscale = pow2f(ex);
            if (bad && tid == 0 && a.status != nullptr) atomicOr(a.status, (int)STATUS_NONFINITE);
        }
        oscale = a.out_scale / rscale;      // power of two: exact
    }
    float res_in = 1.0f, res_rescale = 1.0f;    // res phase: operand prescale 2^a; accumulator factor between the two products' units
    if (res_steps > 0) {
        if (a.res_tot0 != nullptr) {
            bool bad;
            res_in = pow2f(__builtin_amdgcn_readfirstlane(raw_prescale_exp(res_acc, &bad)));
            if (bad && tid == 0 && a.status != nullptr) atomicOr(a.status, (int)STATUS_NONFINITE);
        }
        // 3x3 product: true value = acc * out_scale;  res product: true value = acc * res_scale / res_in  (all powers of two)
        res_rescale = a.out_scale * res_in / a.res_scale;
        oscale = a.res_scale / res_in;
    }
    transform(0);
    if constexpr (WM == 1) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
    }

    TS(TS_PROLOGUE)
    // 16-channel chunks pair two taps per step: lanes kq >= 2 read the tap AFTER the one lanes kq < 2 read, which is 32 bytes
    // further in the halo row (frag_next) or, from a row's last tap to the next row's first, (IW - 2) * 32 (frag_wrap).  With
    // these two per-lane bases every fragment address of every walk is base + an immediate offset (one base per step and row
    // held in a register cost 10 registers per 16-pixel row once the pair walk had 15 distinct steps).
    // (formed here, behind the prologue: four registers fewer across the GroupNorm set-up)
    int frag_next[MT], frag_wrap[MT];
#pragma unroll
    for (int mt = 0; mt < MT; ++mt) {
        frag_next[mt] = frag_base[mt] + (kq >> 1) * 32;
        frag_wrap[mt] = frag_base[mt] + (kq >> 1) * ((IW - KS + 1) * 32);
    }
    int rd_slot = 0;
    half8 xh[MT], xl[MT];
    auto load_x = [&](const int (&xo)[MT], int off) {       // off: a constant once the step loops are unrolled
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            xh[mt] = *reinterpret_cast<const half8*>(img + xo[mt] + off);
            if constexpr (PL == 2) xl[mt] = *reinterpret_cast<const half8*>(img + xo[mt] + off + PLANE);
        }
    };
    // lower lanes tap t0, upper lanes tap t0 + 1 (or, `single`, every lane tap t0: the upper half meets zero weights or is not used)
    auto tap_off = [](int t) { return ((t / KS) * IW + (t % KS)) * 32; };
    // Pair walk: the fragment registers carry a value from one chunk to the next only from the even to the odd chunk of a pair.
    // Everywhere else they are dead at a chunk's end, which the compiler cannot see (the odd chunk's masked load reads them):
    // an empty statement that "defines" them ends their live range there -- no instruction, and no 4*PL*MT registers held
    // through the epilogue.
    auto kill_x = [&]() {
        if constexpr (PAIR) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt) {
                asm volatile("" : "=v"(xh[mt]));
                if constexpr (PL == 2) asm volatile("" : "=v"(xl[mt]));
            }
        }
    };
    // The tap-8 fragments an even chunk leaves for the next chunk's first step.  Only lanes kq < 2 of them are used, so with
    // MT == 2 both 16-pixel rows share ONE register set across the transform: lanes kq >= 2 read row 1's fragment for lanes
    // kq - 2 (same address pattern: a fragment offset depends on kq & 1 only), and v_permlane32_swap moves that half down
    // into xh[1] / xl[1] right before the masked load of the new image.  4 * PL registers held across the transform, not 4 * PL * MT.
    auto load_stash = [&]() {
        constexpr int T8 = (((TAPS - 1) / KS) * IW + (TAPS - 1) % KS) * 32;
        if constexpr (MT == 2) {
            const int so = (kq >> 1) ? frag_base[1] : frag_base[0];
            xh[0] = *reinterpret_cast<const half8*>(img + so + T8);
            if constexpr (PL == 2) xl[0] = *reinterpret_cast<const half8*>(img + so + T8 + PLANE);
        } else {
            load_x(frag_base, T8);
        }
    };
    auto unpack_stash = [&]() {
        if constexpr (MT == 2) {
            typedef unsigned u32x4_ __attribute__((ext_vector_type(4)));
            auto unpack = [](half8& lo, half8& hi) {       // hi[lanes 0..31] <- lo[lanes 32..63]; lo keeps its lanes 0..31
                u32x4_ a = __builtin_bit_cast(u32x4_, lo), b = __builtin_bit_cast(u32x4_, hi);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const auto sw = __builtin_amdgcn_permlane32_swap(a[r], b[r], false, false);
                    a[r] = sw[0]; b[r] = sw[1];
                }
                lo = __builtin_bit_cast(half8, a); hi = __builtin_bit_cast(half8, b);
            };
            unpack(xh[0], xh[1]);
            if constexpr (PL == 2) unpack(xl[0], xl[1]);
        }
    };
    auto mfma_step = [&]() {
        const char* wslot = wring + rd_slot * WSLICE + wfrag_off;
        rd_slot = (rd_slot + 1 == RING) ? 0 : rd_slot + 1;
        half8 wh[NT], wl[NT];
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            wh[nt] = *reinterpret_cast<const half8*>(wslot + nt * WTILE);
            if constexpr (PL == 2) wl[nt] = *reinterpret_cast<const half8*>(wslot + nt * WTILE + 1024);
        }
#ifdef MIDD_DMA_CHECK
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            dma_bad |= has_sent(wh[nt], SENT_W);
            if constexpr (PL == 2) dma_bad |= has_sent(wl[nt], SENT_W);
        }
#endif
#pragma unroll
        for (int mt = 0; mt < MT; ++mt)
#pragma unroll
            for (int nt = 0; nt < NT; ++nt)
                acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[nt], xh[mt], acc[mt][nt], 0, 0, 0);
#if !(defined(C16_ABL) && C16_ABL == 8)  // ablation 8 (wrong results): one MFMA pass instead of three
        if constexpr (PL == 2) {           // the two cross terms of the split product
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[nt], xl[mt], acc[mt][nt], 0, 0, 0);
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt)
                    acc[mt][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[nt], xh[mt], acc[mt][nt], 0, 0, 0);
        }
#endif
    };

    // The activation fragments of a step only depend on the chunk's image (published at the chunk
    // boundary), not on the step's barrier: they are requested first, so their LDS latency overlaps the wait.
    // `first` = first step of a chunk: its barrier is also the one that publishes the freshly transformed
    // image, so the fragments are read after it (WM == 1 has a dedicated barrier after the transform).
    // `merge` (pair walk, first step of an odd chunk): lanes kq < 2 keep the tap-8 fragments of the previous image that the
    // even chunk left in xh / xl; only lanes kq >= 2 read the new image (a divergent load: the LDS instruction count, which
    // the lgkmcnt below counts on, is the same).
    auto k_step = [&](auto with_a, auto merge, bool first, bool first_with_more, int next_chunk, const int (&xo)[MT], int xoff) {
        constexpr bool WITH_A = decltype(with_a)::value;
        constexpr bool MERGE = decltype(merge)::value;
        auto load_frag = [&]() {
            if constexpr (MERGE) { unpack_stash(); if (kq >= 2) load_x(xo, xoff); }
            else load_x(xo, xoff);
        };
#ifdef MIDD_DMA_CHECK_BREAK                // the checker's own test: a wait that is one weight step too permissive must be reported
        constexpr int N = D * PPW + (WITH_A ? APW : 0);
#else
        constexpr int N = (D - 1) * PPW + (WITH_A ? APW : 0);
#endif
        const bool early = (WM == 1) || !first;
        if (early) {
            // One plane: the issue order the lgkmcnt below counts on is PINNED.  The ring slot of the previous step is refilled by
            // ANOTHER wave right after this step's barrier, so this wave's weight reads of that step must have retired before
            // it; "at most PL*MT outstanding" says so only if the fragment reads are the youngest LDS operations.  In the
            // unrolled tap loop the compiler hoisted them above the previous step's last weight read (seen in the ISA of the
            // wide tile): that read then crossed the barrier unretired, and with three workgroups' LDS traffic on a CU the
            // refill could land first -- rare wrong tiles, other ones every run, on the MI355X.  (The two-plane kernel is
            // compiled from the same text; its schedule is left as it is: its ISA is pinned against the parent's.)
            if constexpr (PL == 1) __builtin_amdgcn_sched_barrier(0);
            load_frag();
            // LDS operations retire in order: "at most PL*MT outstanding" = everything older than the
            // fragment reads just issued (the previous step's weight reads) is done
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(%1)" ::"n"(N), "n"(PL * MT) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
        }
        TS(TS_DMAWAIT)                     // diagnostic build: the counted wait alone, then the barrier (TS_WAIT)
        if constexpr (WM != 1) {           // WM == 1: own weights only, no cross-wave hand-off per step
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
#ifdef MIDD_CONV_TIMING
        if (ts_after_epi) { TS(TS_FIRSTWAIT) ts_after_epi = false; } else { TS(TS_WAIT) }
#endif
        if (!early) load_frag();
        issue_w();
        if (first_with_more) issue_a(next_chunk);  // each thread already consumed its own raw slots
        TS(TS_ISSUE)
        mfma_step();
        TS(TS_MFMA)
    };

    // ---- res_conv folded into the tile (ConvArgs::res_*; SURVEY 2.1, DDIMModel.py:126,133) -------------------------------
    // After a tile's 3x3 steps the accumulators are rescaled (power of two) and res_steps more K steps run over the BLOCK
    // INPUT's channels, 32 per step: the 1x1 res_conv.  No halo, no taps, every wave needs only ITS pixels: the B operand comes
    // straight from global memory into registers (lane = (pixel, 8 channels), as conv1x1_f16x3.hip), two steps ahead, through
    // loads the compiler does not track (a tracked load is awaited with vmcnt(0) while LDS-DMA is pending); the weights are
    // further steps of the same ring.  Replaces 15 launches per forward, their output tensors and conv2's residual read.
    // vmcnt bookkeeping per wave, program order:  A(0) A(1) | it 0: W A(2) | it 1: W A(3) | ...   (W = issue_w, PPW pieces;
    // A = RL loads).  Iteration r needs A(r): younger are the W of iteration r-1 (r >= 1) and A(r+1) (if any).  The ring slot
    // of step r was requested D >= 2 iterations (or 3x3 steps) earlier, i.e. before A(r): complete with it.
    constexpr int RL = 2 * MT;                            // untracked 16-byte loads per wave and res step
    constexpr int RG = (MT == 1) ? 2 : 1;                 // res steps per group: the loads of group g+1 fly under the MFMAs of group g
    // every hand-counted vmcnt immediate of this instantiation fits the 6-bit field (k_step, chunk end, res_mfma, res_wait)
    static_assert((D - 1) * PPW + APW <= 63 && D * PPW <= 63 && (D - 1) * PPW + RG * RL <= 63 && RG * PPW <= 63, "vmcnt immediate beyond 63");
    auto res_load = [&](int r, f32x4 (&dst)[MT][2]) {
        const int rc = a.res_C0 + a.res_C1;
        int ch = r * 32 + kq * 8;
        if (ch >= rc) ch = rc - 8;                        // trailing half step: valid dummy, meets zero weights
        const float* src; int nb, cc;               // 8 channels inside one 16-channel block of the blocked layout
        if (ch < a.res_C0) { src = a.res_src0; nb = a.res_C0 >> 4; cc = ch; } else { src = a.res_src1; nb = a.res_C1 >> 4; cc = ch - a.res_C0; }
        src += ((size_t)(b * nb + (cc >> 4)) * (size_t)(a.OH * a.OW)) * 16 + (cc & 15);
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int pp = (wm * MT + mt) * 16 + p16;
            const int py = pp / TW, px = pp - py * TW;
            const int oy = min(oy0 + py, a.OH - 1), ox = min(ox0 + px, a.OW - 1);
            const float* q = src + (size_t)(oy * a.OW + ox) * 16;
#ifdef MIDD_DMA_CHECK
            dst[mt][0] = sent4(SENT_A); dst[mt][1] = sent4(SENT_A);
            asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(dst[mt][0]) : "v"(q) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "+v"(dst[mt][1]) : "v"(q) : "memory");
#else
            asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(dst[mt][0]) : "v"(q) : "memory");
            asm volatile("global_load_dwordx4 %0, %1, off offset:16" : "=&v"(dst[mt][1]) : "v"(q) : "memory");
#endif
        }
    };
    // The raw registers of a group are written by the load statements and named again ("+v") by ONE wait statement: no
    // use of them can be scheduled above the wait.  Loads and wait of a group sit in the SAME loop iteration, so the
    // compiler has no loop-carried copy of them to make before the data has landed (it did, with the raw registers
    // carried across iterations: copies of not-yet-loaded registers, NaN); what crosses iterations are the split
    // operands, ordinary values.
    auto res_wait = [&](f32x4 (&r)[RG][MT][2], auto n_t) {
        constexpr int N = decltype(n_t)::value;
        if constexpr (MT == 2) asm volatile("s_waitcnt vmcnt(%4) ; asm-loads-landed" : "+v"(r[0][0][0]), "+v"(r[0][0][1]), "+v"(r[0][1][0]), "+v"(r[0][1][1]) : "n"(N) : "memory");
        else asm volatile("s_waitcnt vmcnt(%4) ; asm-loads-landed" : "+v"(r[0][0][0]), "+v"(r[0][0][1]), "+v"(r[1][0][0]), "+v"(r[1][0][1]) : "n"(N) : "memory");
    };
    static_assert((MT == 2 && RG == 1) || (MT == 1 && RG == 2), "res_wait names exactly the registers of one group");
    half8 rxh[RG][MT], rxl[RG][MT];                       // split operands of the current group
    auto res_split = [&](int r, f32x4 (&ra)[MT][2], half8 (&oh)[MT], half8 (&ol)[MT]) {
        const bool valid = r * 32 + kq * 8 < a.res_C0 + a.res_C1;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
#ifdef MIDD_DMA_CHECK
            dma_bad |= has_sent(ra[mt][0], SENT_A) | has_sent(ra[mt][1], SENT_A);
#endif
            f32x4 v0 = ra[mt][0] * res_in, v1 = ra[mt][1] * res_in;
            if (!valid) { v0 = (f32x4){0.f, 0.f, 0.f, 0.f}; v1 = v0; }        // keep the dummy finite
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            u32x4 hw, lw;
            unsigned hh, ll;
            planes_pair<PL>(v0[0], v0[1], hh, ll); hw[0] = hh; lw[0] = ll;
            planes_pair<PL>(v0[2], v0[3], hh, ll); hw[1] = hh; lw[1] = ll;
            planes_pair<PL>(v1[0], v1[1], hh, ll); hw[2] = hh; lw[2] = ll;
            planes_pair<PL>(v1[2], v1[3], hh, ll); hw[3] = hh; lw[3] = ll;
            oh[mt] = __builtin_bit_cast(half8, hw);
            ol[mt] = __builtin_bit_cast(half8, lw);
        }
    };
    // one res K step: the ring protocol of k_step (wait for W(step), barrier, refill), operands from registers.
    // in_flight: the next group's RG*RL loads were issued before this step (younger than W(step): they add to the count)
    auto res_mfma = [&](auto in_flight, half8 (&oh)[MT], half8 (&ol)[MT]) {
        constexpr int N = (D - 1) * PPW + (decltype(in_flight)::value ? RG * RL : 0);
        asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(N) : "memory");
        if constexpr (WM != 1) {
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        issue_w();
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) { xh[mt] = oh[mt]; xl[mt] = ol[mt]; }
        mfma_step();
    };
    // vmcnt bookkeeping per wave, program order (W = issue_w: PPW pieces; A(g) = RG*RL loads of group g):
    //   A(0) [wait 0] | group 0: A(1) W .. W [wait RG*PPW] | group 1: A(2) W .. W [wait RG*PPW] | ... | last group: W .. W
    // A step's wait for its ring slot W(s) (requested D steps earlier): younger are W(s+1 .. s+D-1) and the group's A if W(s)
    // was requested before them (the group's i-th step: i < D).
    auto res_phase = [&]() {
        if constexpr (RES) {
            if (res_steps == 0) return;
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) acc[mt][nt] *= res_rescale;
            {
                f32x4 ra[RG][MT][2];
#pragma unroll
                for (int i = 0; i < RG; ++i) res_load(min(i, res_steps - 1), ra[i]);
                res_wait(ra, std::integral_constant<int, 0>{});
#pragma unroll
                for (int i = 0; i < RG; ++i) res_split(i, ra[i], rxh[i], rxl[i]);
            }
            for (int r = 0; r < res_steps; r += RG) {
                const bool more = r + RG < res_steps;
                if (more) {
                    f32x4 ra[RG][MT][2];
#pragma unroll
                    for (int i = 0; i < RG; ++i) res_load(min(r + RG + i, res_steps - 1), ra[i]);     // (a group's missing last step: a duplicate, unused)
                    // the group's loads are younger than W(step) only while that slot was requested BEFORE them, i.e. for the
                    // group's steps i < D (round 4: with a two-slot ring, D = 1, the second step's slot is requested after the
                    // loads and nothing younger than it may stay outstanding -- found by tests/test_dma_protocol_cpu.py; the
                    // three two-slot tiles with MT = 1 are never picked for the default network)
                    res_mfma(std::true_type{}, rxh[0], rxl[0]);
                    if constexpr (RG == 2) {
#ifdef MIDD_DMA_CHECK_OLD_RES              // the checker's second self-test: round 3's count for this step (the loads counted although they are older)
                        if (r + 1 < res_steps) res_mfma(std::true_type{}, rxh[1], rxl[1]);
#else
                        if (r + 1 < res_steps) res_mfma(std::integral_constant<bool, (1 < D)>{}, rxh[1], rxl[1]);
#endif
                    }
                    res_wait(ra, std::integral_constant<int, RG * PPW>{});
#pragma unroll
                    for (int i = 0; i < RG; ++i) res_split(r + RG + i, ra[i], rxh[i], rxl[i]);
                } else {
#pragma unroll
                    for (int i = 0; i < RG; ++i)
                        if (r + i < res_steps) res_mfma(std::false_type{}, rxh[i], rxl[i]);
                }
            }
            kill_x();
        }
    };

    // ---- epilogue (per tile) ------------------------------------------------------------------
    // GroupNorm partial sums of the output run across ALL tiles of this (persistent) workgroup and are
    // published once at the end: one row per (workgroup, wave) instead of one per (tile, wave).  Per tile the
    // 16 pixel lanes are folded (fixed order -> deterministic) and lanes p16 == 0 add into the wave's LDS row.
    // GroupNorm partial sums of the output: each lane keeps the sums of ITS pixels (fixed (pixel lane, cout quad) of every
    // tile it walks) in registers across all tiles of this persistent workgroup; the 16 pixel lanes are folded (DPP row
    // sums, fixed order) and the waves combined through LDS ONCE, at the end.  (Doing the DPP fold and an LDS
    // read-modify-write per tile cost 9 % of the whole sampler: ablation with the statistics removed.)
    f32x4 ssum[NT], ssq[NT];
#pragma unroll
    for (int nt = 0; nt < NT; ++nt) { ssum[nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; ssq[nt] = (f32x4){0.f, 0.f, 0.f, 0.f}; }
    auto epilogue = [&]() {
        // The residual operand comes through loads the compiler does not track (a tracked load is awaited with vmcnt(0) while
        // LDS-DMA traffic is pending, stats_common.h), ALL of the tile's MT*NT at once and awaited once: vmcnt counts stores
        // too, so a wait per 16-pixel row (round 2) also waited for the previous row's output stores to retire.  The K loop's
        // fragment registers are dead here, which is what makes room for them.
        f32x4 rres[MT][NT];
        size_t obase[MT];
        bool rowok[MT];
        const size_t ohw = (size_t)a.OH * a.OW;
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            const int pp = (wm * MT + mt) * 16 + p16;
            const int py = pp / TW, px = pp - py * TW;
            const int oy = oy0 + py, ox = ox0 + px;
            rowok[mt] = oy < a.OH && ox < a.OW;
            // blocked output [B][Cout/16][OH][OW][16]: the 16 pixel lanes x 4 cout quads of an MFMA tile write one contiguous KiB
            obase[mt] = (((size_t)b * (a.Cout >> 4) + ntile0) * ohw + (size_t)(min(oy, a.OH - 1) * a.OW + min(ox, a.OW - 1))) * 16 + kq * 4;
        }
        if (a.resid != nullptr) {
#pragma unroll
            for (int mt = 0; mt < MT; ++mt)
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {     // (rows beyond the image: a valid, clamped address; never stored)
#ifdef MIDD_DMA_CHECK
                    rres[mt][nt] = sent4(SENT_A);
                    asm volatile("global_load_dwordx4 %0, %1, off" : "+v"(rres[mt][nt]) : "v"(a.resid + obase[mt] + nt * ohw * 16) : "memory");
#else
                    asm volatile("global_load_dwordx4 %0, %1, off" : "=&v"(rres[mt][nt]) : "v"(a.resid + obase[mt] + nt * ohw * 16) : "memory");
#endif
                }
            // one statement names every destination: nothing that uses (or copies) them can be scheduled above the wait
            if constexpr (MT == 2 && NT == 3) asm volatile("s_waitcnt vmcnt(0) ; asm-loads-landed" : "+v"(rres[0][0]), "+v"(rres[0][1]), "+v"(rres[0][2]), "+v"(rres[1][0]), "+v"(rres[1][1]), "+v"(rres[1][2]) :: "memory");
            else if constexpr (MT == 2 && NT == 2) asm volatile("s_waitcnt vmcnt(0) ; asm-loads-landed" : "+v"(rres[0][0]), "+v"(rres[0][1]), "+v"(rres[1][0]), "+v"(rres[1][1]) :: "memory");
            else if constexpr (MT == 2 && NT == 1) asm volatile("s_waitcnt vmcnt(0) ; asm-loads-landed" : "+v"(rres[0][0]), "+v"(rres[1][0]) :: "memory");
            else if constexpr (MT == 1 && NT == 3) asm volatile("s_waitcnt vmcnt(0) ; asm-loads-landed" : "+v"(rres[0][0]), "+v"(rres[0][1]), "+v"(rres[0][2]) :: "memory");
            else if constexpr (MT == 1 && NT == 2) asm volatile("s_waitcnt vmcnt(0) ; asm-loads-landed" : "+v"(rres[0][0]), "+v"(rres[0][1]) :: "memory");
            else asm volatile("s_waitcnt vmcnt(0) ; asm-loads-landed" : "+v"(rres[0][0]) :: "memory");
        }
#pragma unroll
        for (int mt = 0; mt < MT; ++mt) {
            if (rowok[mt]) {
#pragma unroll
                for (int nt = 0; nt < NT; ++nt) {
                    const f32x4 add = *reinterpret_cast<const f32x4*>(add_lds + (wn * NT + nt) * 16 + kq * 4);
                    f32x4 v = acc[mt][nt] * oscale + add;
#ifdef MIDD_DMA_CHECK
                    if (a.resid != nullptr) dma_bad |= has_sent(rres[mt][nt], SENT_A);
#endif
                    if (a.resid != nullptr) v += rres[mt][nt];
                    *reinterpret_cast<f32x4*>(a.out + obase[mt] + nt * ohw * 16) = v;
#if !(defined(C16_ABL) && C16_ABL == 1)  // ablation 1 (wrong results): no statistics of the output
                    ssum[nt] += v; ssq[nt] += v * v;
#endif
                }
            }
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) acc[mt][nt] = (f32x4){0.f, 0.f, 0.f, 0.f};
        }
    };
    // the waves' LDS rows are folded over wm in a fixed order after a barrier; the workgroup's per-channel sums go to
    // the tensor's totals with exact integer atomics (stats_common.h)
    auto publish_stats = [&]() {
        if (a.stat_tot == nullptr) return;
#if defined(C16_ABL) && (C16_ABL == 1 || C16_ABL == 9)      // ablation 9 (wrong results): sums accumulated, never published
        return;
#endif
        float* const my_stat = stat_lds + wave * (2 * NT * 16) + kq * 4;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
#pragma unroll
            for (int e = 0; e < 4; ++e) { ssum[nt][e] = row16_sum(ssum[nt][e]); ssq[nt][e] = row16_sum(ssq[nt][e]); }
            if (p16 == 0) {                     // raw stores: see stat_publish
                lds_store_raw(my_stat + nt * 16, ssum[nt]);
                lds_store_raw(my_stat + NT * 16 + nt * 16, ssq[nt]);
            }
        }
        constexpr int ROWF = 2 * NT * 16;                              // floats of one wave's row
        constexpr int NCOL = WN * NT * 16;                             // channels of this workgroup's slice
        // the waves' rows are folded over wm in a fixed order inside stat_publish (its first barrier publishes them)
        auto fold = [&](int i) {
            const int which = i / NCOL, col = i - which * NCOL;
            const int wn_i = col / (NT * 16), c = col - wn_i * (NT * 16);
            float t = 0.f;
#pragma unroll
            for (int m = 0; m < WM; ++m) t += stat_lds[(m * WN + wn_i) * ROWF + which * (NT * 16) + c];
            return t;
        };
        static_assert(G::RAW_BYTES + G::IMG_BYTES + RING * WSLICE >= (NCOL + 2) * STAT_WORDS * 8, "block accumulators in the staging buffers (raw, image, ring: contiguous, idle here)");
        // the landing buffer has been idle for every wave since the last transform; the image / ring behind it may still be
        // read by a wave in its last steps, so accumulators that spill into them wait for everybody first
        if constexpr (G::RAW_BYTES < (NCOL + 2) * STAT_WORDS * 8) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            __builtin_amdgcn_s_barrier();
            asm volatile("" ::: "memory");
        }
        stat_publish(a.stat_tot, b, a.Cout, a.stat_bs, a.stat_rep, (blockIdx.x - b * a.wgs_per_img) % a.stat_rep, ntile_wg * 16, NCOL,
                     fold, reinterpret_cast<stat_word*>(raw), tid, NTHREADS);
    };

    // ---- tile / chunk loop -----------------------------------------------------------------------
    for (;;) {
        const int next_tile = trem + a.wgs_per_img;
        const bool has_next_tile = next_tile < tiles_per_img;
        for (int c = 0; c < nchunks; ++c) {
            const bool more_in_tile = (c + 1 < nchunks);
            const bool more = more_in_tile || has_next_tile;
            const int next_chunk = more_in_tile ? c + 1 : 0;
            const bool full = (CB == 2) && (2 * c + 1 < nblk);
            // the staging geometry switches to the next tile right before its first chunk is requested
            // (every transform of the current tile is done by then; the epilogue does not use it)
            if (!more_in_tile && has_next_tile) set_tile(next_tile);
            // pair walk: 0 = a chunk of its own (5 steps), 1 = the even chunk of a pair (4 steps + the tap-8 stash), 2 = the odd one
            const int walk = !PAIR ? 0 : (c & 1) ? 2 : more_in_tile ? 1 : 0;
            auto run_chunk = [&](auto more_t, auto walk_t) {
                constexpr bool MORE = decltype(more_t)::value;
                constexpr int WALK = decltype(walk_t)::value;
                if constexpr (WALK != 0) {
#pragma unroll
                    for (int j = 0; j < (WALK == 1 ? HSTEPS - 1 : HSTEPS); ++j) {
                        // even: taps (2j | 2j+1) of this block; odd: (8 of the previous block, in registers | 0), then (2j-1 | 2j)
                        const int t0 = (WALK == 1) ? 2 * j : 2 * j - 1;
                        if (j == 0 && WALK == 2)         k_step(std::false_type{}, std::true_type{}, true, MORE, next_chunk, frag_base, tap_off(0));
                        else if (MORE && j >= 1 && j <= D) k_step(std::true_type{}, std::false_type{}, false, false, next_chunk, t0 % KS == KS - 1 ? frag_wrap : frag_next, tap_off(t0));
                        else                             k_step(std::false_type{}, std::false_type{}, j == 0, MORE && j == 0, next_chunk, t0 % KS == KS - 1 ? frag_wrap : frag_next, tap_off(t0));
                    }
                    if constexpr (WALK == 1) {            // tap 8 of this image, for the next chunk's first step (all lanes read; kq < 2 keep it)
                        load_stash();
                    }
                    if constexpr (WALK == 2) kill_x();
                    return;
                }
                if (full) {
#pragma unroll
                    for (int tap = 0; tap < TAPS; ++tap) {
                        const int dy = tap / KS, dx = tap - dy * KS;
                        const int xoff = (dy * IW + dx) * 32;
                        if (MORE && tap >= 1 && tap <= D) k_step(std::true_type{}, std::false_type{}, false, false, next_chunk, frag_full, xoff);
                        else                              k_step(std::false_type{}, std::false_type{}, tap == 0, MORE && tap == 0, next_chunk, frag_full, xoff);
                    }
                } else {
#pragma unroll
                    for (int hs = 0; hs < HSTEPS; ++hs) {
                        // taps (2 hs | 2 hs + 1); the padded half of the last step has zero weights: every lane reads the last tap
                        const int t0 = 2 * hs;
                        const int (&xb)[MT] = (t0 + 1 >= TAPS) ? frag_base : (t0 % KS == KS - 1) ? frag_wrap : frag_next;
                        if (MORE && hs >= 1 && hs <= D) k_step(std::true_type{}, std::false_type{}, false, false, next_chunk, xb, tap_off(t0));
                        else                            k_step(std::false_type{}, std::false_type{}, hs == 0, MORE && hs == 0, next_chunk, xb, tap_off(t0));
                    }
                }
                kill_x();
            };
            if (more) {
                if constexpr (PAIR) {
                    if (walk == 1)      run_chunk(std::true_type{}, std::integral_constant<int, 1>{});
                    else if (walk == 2) run_chunk(std::true_type{}, std::integral_constant<int, 2>{});
                    else                run_chunk(std::true_type{}, std::integral_constant<int, 0>{});
                } else {
                    run_chunk(std::true_type{}, std::integral_constant<int, 0>{});
                }
                if (!more_in_tile) { res_phase(); TS(TS_RES) }         // the tile's 3x3 steps are done: the folded res_conv's steps
                // every wave is done reading the image, and A(next) (older than the last min(steps after it, D)
                // weight groups) has landed, before the image is rewritten
                // vmcnt(min(after, D) * PPW), derived at the head of the K loop; an `after` that cannot occur below D costs nothing
                const int after = (full ? TAPS : walk == 1 ? HSTEPS - 1 : HSTEPS) - 1 + (more_in_tile ? 0 : res_steps);
                // (one arm per value below D; tests/test_pair_walk_cpu.py reads these arms and replays them)
                if (after >= D) wait_vm_and_barrier<D * PPW>();
                else if (after == 4) wait_vm_and_barrier<cmin(4, D) * PPW>();
                else if (after == 3) wait_vm_and_barrier<cmin(3, D) * PPW>();
                else if (after == 2) wait_vm_and_barrier<cmin(2, D) * PPW>();
                else if (after == 1) wait_vm_and_barrier<cmin(1, D) * PPW>();
                else wait_vm_and_barrier<0>();
                TS(TS_CHUNK_WAIT)
                if (!more_in_tile) {                    // tile finished: store it, move to the next one
                    epilogue();
                    trem = next_tile;
                    oy0 = (trem / a.tiles_x) * TH; ox0 = (trem % a.tiles_x) * TW;
                    TS(TS_EPILOGUE)
#ifdef MIDD_CONV_TIMING
                    ts_after_epi = true;
#endif
                }
#if !(defined(C16_ABL) && C16_ABL == 5)  // ablation 5 (wrong results): no transform in the loop
                transform(next_chunk);
#endif
                TS(TS_TRANSFORM)
                if constexpr (WM == 1) {        // steps have no barrier of their own: publish the new image here
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_s_barrier();
                    asm volatile("" ::: "memory");
                }
            } else {
                if constexpr (PAIR) {               // (the even chunk of a pair is never a tile's last)
                    if (walk == 2) run_chunk(std::false_type{}, std::integral_constant<int, 2>{});
                    else           run_chunk(std::false_type{}, std::integral_constant<int, 0>{});
                } else {
                    run_chunk(std::false_type{}, std::integral_constant<int, 0>{});
                }
                res_phase();
                TS(TS_RES)
            }
        }
        if (!has_next_tile) break;
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // the weight refills issued past the last step
    TS(TS_CHUNK_WAIT)
    epilogue();
    TS(TS_EPILOGUE)
    publish_stats();
#ifdef MIDD_DMA_CHECK
    if (dma_bad && a.status != nullptr) atomicOr(a.status, (int)STATUS_DMA_EARLY);
#endif
    TS(TS_PUBLISH)
#ifdef MIDD_CONV_TIMING
    if (tid == 0) {
        ts_acc[TS_TOTAL] = ts_last - ts_t0;
        ts_acc[TS_REAL] = __builtin_amdgcn_s_memrealtime() - ts_r0;
        ts_acc[TS_WGS] = 1;
        for (int k = 0; k < TS_N; ++k) atomicAdd(&g_conv_timing[a.dbg_slot][k], ts_acc[k]);
    }
#endif
}
