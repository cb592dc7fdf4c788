// The body of the fp16-MFMA fused attention kernel (attention_f16x3.hip describes it).  attention_f16x3.hip includes this text
// TWICE (conv_mfma_f16x3_body.h says why it is textual):
//   MIDD_ATT16_KERNEL = attention_f16x3_kernel, MIDD_ATT16_PL = 2   q, K, V, P as hi | lo, three MFMAs per product
//   MIDD_ATT16_KERNEL = attention_f16_kernel,   MIDD_ATT16_PL = 1   compute "f16": QK^T and PV with one MFMA each, q rounded on load,
//                                                                  P rounded in registers with the same 2^10 scale, one-plane K / V images
#if !defined(MIDD_ATT16_KERNEL) || !defined(MIDD_ATT16_PL)
#error "include from attention_f16x3.hip with MIDD_ATT16_KERNEL and MIDD_ATT16_PL defined"
#endif

template <int D>
__global__ __launch_bounds__(256, 2)
void MIDD_ATT16_KERNEL(const float* __restrict__ q, const _Float16* __restrict__ Kp, const _Float16* __restrict__ Vp,
                       float* __restrict__ part_o, float* __restrict__ part_ml,
                       int N, int Npad, int C, float qscale, int ksplit, int tiles_per_split) {
    constexpr int PL = MIDD_ATT16_PL;
    static_assert(PL == 1 || PL == 2, "planes");
    using G = Att16Geom<D, PL>;
    constexpr int DC = D / 32;                 // 32-wide k chunks of the head dimension (QK^T)
    constexpr int DT = D / 16;                 // 16-row output tiles of O^T
    constexpr int QM = A16_QW / 16;            // 16-query column tiles per wave
    constexpr int KB = A16_KT / 16;            // 16-key blocks per tile
    static_assert(D % 32 == 0 && KB == 2, "head_dim must be a multiple of 32; one 32-key pair-block per tile");
    extern __shared__ __attribute__((aligned(16))) char lds[];            // two stages of [K hi | K lo | V hi | V lo], rows = keys

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l16 = lane & 15, kq = lane >> 4;
    // XCD-aware mapping.  Workgroups are dealt round-robin to the 8 XCDs in linear order (x fastest), each XCD has its own
    // 4 MB L2, and every workgroup of a (sample, head) pair streams that pair's whole K / V image (3.1 MB at N = 4096):
    // in launch order a pair's workgroups land on all XCDs and every L2 sees every pair (25 MB at B = 4) -- the K / V tiles
    // come from the fabric each time (786 MB per launch at N = 4096).  Remapped, a pair's workgroups share ONE XCD (8 or
    // more pairs) or an equal share of them (1, 2, 4 pairs), and its image stays in that L2.
    const int heads = gridDim.y;
    int bx = blockIdx.x, pair = blockIdx.y + gridDim.y * blockIdx.z;
    {
        const int X = gridDim.x, P = gridDim.y * gridDim.z;
        const int L = blockIdx.x + X * pair, xcd = L & 7, k = L >> 3;
        if (P % 8 == 0) { pair = xcd + 8 * (k / X); bx = k % X; }
        else if (8 % P == 0 && X % (8 / P) == 0) { const int r = 8 / P; pair = xcd / r; bx = k * r + xcd % r; }
    }
    const int head = pair % heads, b = pair / heads;
    const int qb = bx / ksplit, ks = bx - qb * ksplit;
    const int q0 = qb * A16_QB + wave * A16_QW;
    const float* base = q + (size_t)b * N * C;                       // q: fp32 [B][N][C] (the qkv projection's epilogue)
    const int qcol = head * D;
    const char* gk = reinterpret_cast<const char*>(Kp + ((size_t)(b * heads + head) * PL) * Npad * D);    // [hi|lo (PL planes)][Npad][D]
    const char* gv = reinterpret_cast<const char*>(Vp + ((size_t)(b * heads + head) * PL) * Npad * D);
    const int ntiles = (N + A16_KT - 1) / A16_KT;
    const int t_begin = ks * tiles_per_split, t_end = min(ntiles, t_begin + tiles_per_split);

    // ---- DMA plan: piece p (1 KiB of the stage image) = chunks 64p .. 64p+63; this lane's chunk -> global source ----
    // chunk c = ((plane4 * 32 + key) * KCH + ch): plane4 = K hi, K lo, V hi, V lo; ch >= D/8 is row padding (dummy source)
    const char* src[G::PPW];
    int adv[G::PPW];                           // bytes the source moves per tile
#pragma unroll
    for (int i = 0; i < G::PPW; ++i) {
        const int piece = wave + 4 * i;
        const int c = piece * 64 + lane;
        const char* s = gk; int a = 0;
        if (c < G::CHUNKS) {
            const int plane4 = c / (A16_KT * G::KCH), rem = c - plane4 * (A16_KT * G::KCH);
            const int key = rem / G::KCH, ch = rem - key * G::KCH;
            if (ch < D / 8) {
                s = (plane4 < PL ? gk : gv) + ((size_t)(plane4 & (PL - 1)) * Npad + key) * (D * 2) + ch * 16;
                a = A16_KT * D * 2;
            }
        }
        src[i] = s + (size_t)t_begin * a; adv[i] = a;                     // pad chunks: a valid dummy source, never read back
    }
    auto issue = [&](int stage) {
        char* dst = lds + stage * G::STAGE;
#pragma unroll
        for (int i = 0; i < G::PPW; ++i) {
            const int piece = wave + 4 * i;
            if (piece < G::PIECES) att_dma16(src[i], dst + piece * 1024);
            src[i] += adv[i];
        }
    };
    if (t_begin < t_end) issue(0);

    // ---- Q^T fragments: lane holds Q[q0 + 16qm + l16][32c + 8kq + j] * scale*log2(e) * 2^4, split hi/lo ----
    half8 qh[QM][DC], ql[QM][DC];
#pragma unroll
    for (int qm = 0; qm < QM; ++qm) {
        const int qi = q0 + qm * 16 + l16;
#pragma unroll
        for (int c = 0; c < DC; ++c) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 v = {0.f, 0.f, 0.f, 0.f};
                if (qi < N) v = *reinterpret_cast<const f32x4*>(base + (size_t)qi * C + qcol + c * 32 + kq * 8 + h * 4);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    _Float16 hi, lo;
                    split1(v[e] * (qscale * A16_QKV_SCALE), hi, lo);      // (one plane: lo is dead code)
                    qh[qm][c][h * 4 + e] = hi; ql[qm][c][h * 4 + e] = lo;
                }
            }
        }
    }

    f32x4 o[QM][DT];
#pragma unroll
    for (int qm = 0; qm < QM; ++qm)
#pragma unroll
        for (int t = 0; t < DT; ++t) o[qm][t] = (f32x4){0.f, 0.f, 0.f, 0.f};
    float m[QM], l[QM];
#pragma unroll
    for (int qm = 0; qm < QM; ++qm) { m[qm] = -INFINITY; l[qm] = 0.f; }

    const int koff = l16 * G::KROW + kq * 16;                 // K fragment: row = key l16 of the block, 8 halfs at d = 32c + 8kq
    // V^T fragment by the transposing read: the 16 lanes of group kq read the block keys 4kq .. 4kq+3 (+16: second half)
    // x d 16t .. 16t+15; lane 4r+p supplies the address of row (key) r, columns 4p .. 4p+3, and lane l16 receives column
    // d = 16t + l16 of the four keys -- the A operand V^T[d][keys 4kq.., 16+4kq..] of the permuted-k PV product
    const int voff = (kq * 4 + (l16 >> 2)) * G::KROW + (l16 & 3) * 8;
    typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    auto tr_read = [&](const char* p) {
        return __builtin_bit_cast(half4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4*)(p)));
    };

    for (int t = t_begin; t < t_end; ++t) {
        const int stage = (t - t_begin) & 1;
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");      // this wave's pieces of tile t have landed (the Q loads too)
        __builtin_amdgcn_s_barrier();                         // ... everybody's; and everybody is done reading the other stage
        asm volatile("" ::: "memory");
        if (t + 1 < t_end) issue(stage ^ 1);
        const char* Kh = lds + stage * G::STAGE;
        const char* Vh = Kh + PL * G::KPLANE;
        const int kt0 = t * A16_KT;

        // S^T = K . Q^T (x 2^8): rows = keys, cols = queries
        f32x4 st[QM][KB];
#pragma unroll
        for (int kb = 0; kb < KB; ++kb) {
#pragma unroll
            for (int qm = 0; qm < QM; ++qm) st[qm][kb] = (f32x4){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int c = 0; c < DC; ++c) {
                const int off = kb * 16 * G::KROW + koff + c * 64;
                const half8 kh = *reinterpret_cast<const half8*>(Kh + off);
                half8 kl{};
                if constexpr (PL == 2) kl = *reinterpret_cast<const half8*>(Kh + G::KPLANE + off);
#pragma unroll
                for (int qm = 0; qm < QM; ++qm) {
                    st[qm][kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, qh[qm][c], st[qm][kb], 0, 0, 0);
                    if constexpr (PL == 2) {
                        st[qm][kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh, ql[qm][c], st[qm][kb], 0, 0, 0);
                        st[qm][kb] = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl, qh[qm][c], st[qm][kb], 0, 0, 0);
                    }
                }
            }
        }

        // online softmax (base-2 domain); lane: query l16 of tile qm, keys kt0 + 16kb + 4kq + r.  The kernel is bound by the
        // vector ALU, not by the MFMAs (round 2: ~300 vector instructions per 72 MFMAs), so: the key-bound mask only in
        // the tile that crosses N, the 2^10 operand prescale of P folded into the exponent, and O rescaled only when some
        // lane's running maximum moved (after the first tiles it rarely does).
        const bool tail = kt0 + A16_KT > N;                   // uniform
        half8 ph[QM], pl[QM];
#pragma unroll
        for (int qm = 0; qm < QM; ++qm) {
            float tmax = -INFINITY;
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                st[qm][kb] = st[qm][kb] * (1.0f / (A16_QKV_SCALE * A16_QKV_SCALE));
                if (tail) {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (kt0 + kb * 16 + kq * 4 + r >= N) st[qm][kb][r] = -INFINITY;
                }
#pragma unroll
                for (int r = 0; r < 4; ++r) tmax = fmaxf(tmax, st[qm][kb][r]);
            }
            tmax = fmaxf(tmax, __shfl_xor(tmax, 16));
            tmax = fmaxf(tmax, __shfl_xor(tmax, 32));
            const float m_new = fmaxf(m[qm], tmax);           // finite: the first key of every tile is < N
            const float alpha = __builtin_amdgcn_exp2f(m[qm] - m_new);
            const float mshift = m_new - A16_P_SHIFT;         // exp2(s - mshift) = 2^10 exp2(s - m_new): P arrives prescaled
            float psum = 0.f;
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            u32x4 phw, plw;
#pragma unroll
            for (int kb = 0; kb < KB; ++kb) {
                float pv[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) { pv[r] = __builtin_amdgcn_exp2f(st[qm][kb][r] - mshift); psum += pv[r]; }
                unsigned hh, ll;
                att_planes_pair<PL>(pv[0], pv[1], hh, ll); phw[kb * 2] = hh; plw[kb * 2] = ll;
                att_planes_pair<PL>(pv[2], pv[3], hh, ll); phw[kb * 2 + 1] = hh; plw[kb * 2 + 1] = ll;
            }
            ph[qm] = __builtin_bit_cast(half8, phw); pl[qm] = __builtin_bit_cast(half8, plw);
            psum += __shfl_xor(psum, 16);
            psum += __shfl_xor(psum, 32);
            l[qm] = l[qm] * alpha + psum;                     // in units of 2^-10 (undone once, after the loop)
            m[qm] = m_new;
            if (__builtin_amdgcn_ballot_w64(alpha != 1.0f) != 0ull) {
#pragma unroll
                for (int tt = 0; tt < DT; ++tt) o[qm][tt] *= alpha;
            }
        }

        // O^T += V^T . P^T over the tile's 32 keys
#pragma unroll
        for (int tt = 0; tt < DT; ++tt) {
            const char* vp = Vh + voff + tt * 32;
            const half4 vh0 = tr_read(vp), vh1 = tr_read(vp + 16 * G::KROW);
            half8 vh, vl{};
#pragma unroll
            for (int e = 0; e < 4; ++e) { vh[e] = vh0[e]; vh[4 + e] = vh1[e]; }
            if constexpr (PL == 2) {
                const half4 vl0 = tr_read(vp + G::KPLANE), vl1 = tr_read(vp + G::KPLANE + 16 * G::KROW);
#pragma unroll
                for (int e = 0; e < 4; ++e) { vl[e] = vl0[e]; vl[4 + e] = vl1[e]; }
            }
#pragma unroll
            for (int qm = 0; qm < QM; ++qm) {
                o[qm][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, ph[qm], o[qm][tt], 0, 0, 0);
                if constexpr (PL == 2) {
                    o[qm][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh, pl[qm], o[qm][tt], 0, 0, 0);
                    o[qm][tt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl, ph[qm], o[qm][tt], 0, 0, 0);
                }
            }
        }
    }

    // O^T accumulator: col = query l16, row = d = 16t + 4kq + r.  Partials (m, l, unnormalised O^T x 2^14) of this split;
    // the output projection combines the splits (conv1x1_f16x3.hip, ATT_PART_IN), also when there is only one.
#pragma unroll
    for (int qm = 0; qm < QM; ++qm) {
        l[qm] *= (1.0f / A16_P_SCALE);                        // exact: back to the unscaled row sum
        const int qi = q0 + qm * 16 + l16;
        if (qi >= N) continue;
        float* orow = part_o + (((size_t)ks * gridDim.z + b) * N + qi) * C + head * D + kq * 4;
#pragma unroll
        for (int tt = 0; tt < DT; ++tt) *reinterpret_cast<f32x4*>(orow + tt * 16) = o[qm][tt];
        if (kq == 0) {
            float* ml = part_ml + ((((size_t)ks * gridDim.z + b) * heads + head) * N + qi) * 2;
            ml[0] = m[qm]; ml[1] = l[qm];
        }
    }
}
