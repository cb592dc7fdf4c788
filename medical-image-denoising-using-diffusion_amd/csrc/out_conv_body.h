// The out_conv kernel's text (out_conv.hip), compiled twice: MIDD_OUT_KERNEL = out_conv_kernel with MIDD_OUT_SEEDED 0 (the
// noise term of the sampler update, if any, is read from a.noise) and out_conv_seeded_kernel with MIDD_OUT_SEEDED 1 (the term is
// drawn in the update from a.seed / a.sample_offset / a.iter: step_noise_common.h -- no noise tensor exists, 4 bytes per pixel
// less are read; sample b of the launch is virtual sample a.v0 + b of an ensemble of a.members draws per image, image-major, or
// -- a.tiles_x != 0 -- of a.members tiles per image, whose noise is indexed by the pixel's place in the whole image).
// Two kernels from one text rather than one template argument more: the unseeded kernels keep their symbols (mi_profile_end,
// plan dumps) and compile to exactly what they were (instruction mix, registers: profiles/step_noise_isa.txt).
// A third compile, MIDD_OUT_SLOTS 1 = out_conv_slots_kernel (mi_denoise_slots): the update's coefficients, the noise counter words
// and whether the sample is updated at all come from the sample's SlotRec (midd_internal.h) instead of the arguments -- every
// sample of the launch is at its own timestep.  b is per workgroup, so the record is read with scalar loads; the workgroups of
// an idle slot leave at once: nothing is staged, drawn or written.  The other two compiles do not see a token of it.
// The record also carries the member word and the (pitch, plane, origin) frame of the element index (mi_denoise_slots_virtual):
// a slot draws what a member of mi_denoise_ensemble or a tile of mi_denoise_tiled draws.
// Two more, MIDD_OUT_DDIM 1 = out_conv_ddim_kernel (MIDD_OUT_SEEDED 0) and out_conv_ddim_seeded_kernel (1): the DDIM(eta) update of
// include/midd.h (THE DDIM UPDATE) in the place of the reference's, its coefficients in a kernel argument of their own (DdimCoef,
// scalar loads).  The three compiles above do not see a token of it either.
// A sixth, MIDD_OUT_DPM 1 = out_conv_dpm_kernel: the second-order multistep update of include/midd.h (THE DPMPP2M UPDATE) -- the
// DDIM update at eta = 0 plus g * (x0 - x0_prev) -- its coefficients in a DpmCoef argument (scalar loads) and two more pointers,
// the previous iteration's predicted image (read) and this one's (written).  The five compiles above do not see a token of it.
// A seventh, MIDD_OUT_SLOTS_RULE 1 = out_conv_slots_rule_kernel (mi_denoise_slots_rule): the DDIM / DPMPP2M blocks below with every
// per-sample scalar from the sample's SlotRuleRec (midd_internal.h), the draw of the slots compile, and one history pointer, null
// under the DDIM rule, read and written in place.  One compile for both rules.  The six compiles above do not see a token of it.
template <int IC>
__global__ __launch_bounds__(256)
void MIDD_OUT_KERNEL(const OutConvArgs a, const float* __restrict__ wglob /* == a.w: a restrict parameter of its own, so that uniform reads become scalar loads */
#if MIDD_OUT_SLOTS
                     , const SlotRec* __restrict__ slots /* [a.B] */
#endif
#if MIDD_OUT_DDIM
                     , const DdimCoef k
#endif
#if MIDD_OUT_DPM
                     , const DpmCoef k, const float* x0_prev, float* x0_out /* [a.B, ic, H, W]; may be one address: not restrict */
#endif
#if MIDD_OUT_SLOTS_RULE
                     , const SlotRuleRec* __restrict__ slots /* [a.B] */, const int clip_x0, float* x0_hist /* [a.B, ic, H, W] or null; read and written: not restrict */
#endif
                     ) {
    __shared__ __attribute__((aligned(16))) float tile[OC_I * OC_I * OC_PS];
    static_assert(sizeof(tile) == out_conv_static_lds_bytes(), "out_conv_lds_bytes (midd_internal.h) counts this tile");
    // No aligned(16) on purpose: it was written here and never took effect.  hipcc fixes the alignment of an `extern __shared__`
    // array where a function that uses it is first emitted, and while this text shared a translation unit with in_conv_kernel
    // that was in_conv_kernel's plain `float wl[]`.  The recorded instruction streams (profiles/step_noise_isa.txt;
    // tests/test_ensemble_cpu.py: 8043 instructions for IC = 0) are those of a 4-byte aligned array, pairs of ds_read2_b32.  With
    // the attribute in force the five IC = 0 kernels read with ds_read_b128 instead: a change that needs its own measurement.
    extern __shared__ float wl[];                                    // [ic][9][C], then [2][C] GroupNorm scale / shift of this sample: out_conv_dynamic_lds_bytes
    const int ic = IC ? IC : a.ic;
    const int tid = threadIdx.x;
    const int tx = tid & 15, ty = tid >> 4;
    float* const gnp = wl + ic * 9 * a.C;
    const int tiles_x = (a.W + OC_T - 1) / OC_T, tiles_y = (a.H + OC_T - 1) / OC_T;
    const int b = blockIdx.x / (tiles_x * tiles_y);
    const int trem = blockIdx.x - b * tiles_x * tiles_y;
    const int oy0 = (trem / tiles_x) * OC_T, ox0 = (trem % tiles_x) * OC_T;
    const int C = a.C;
#if MIDD_OUT_SLOTS
    const SlotRec rec = slots[b];
    if (!rec.active) return;                      // idle slot: x[b] keeps its bits (whole workgroup, before any barrier)
#endif
#if MIDD_OUT_SLOTS_RULE
    const SlotRuleRec rec = slots[b];
    if (!rec.active) return;                      // idle slot: x[b] and x0_hist[b] keep their bits (whole workgroup, before any barrier)
#endif
    if constexpr (IC == 0) for (int i = tid; i < ic * 9 * C; i += 256) wl[i] = a.w[i];     // (IC > 0 reads the weights through scalar loads)

    float acc[4] = {0.f, 0.f, 0.f, 0.f};          // ic <= 4 output channels
    // Staging, round 3: a thread's slots (halo pixel, channel quad) are the same for every 16-channel chunk, so their
    // addresses are formed once, branch-free (clamped; out-of-image and surplus slots load a valid dummy and store
    // zeros), and the NEXT chunk's quads are requested before this chunk's taps: the loads fly under the arithmetic.
    constexpr int NSL = (OC_I * OC_I * 4 + 255) / 256;
    unsigned soff[NSL];                           // float offset of the slot's quad from the chunk's base
    unsigned live = 0;                            // bit s: slot exists and lies in the image
#pragma unroll
    for (int s = 0; s < NSL; ++s) {
        const int slot = min(tid + s * 256, OC_I * OC_I * 4 - 1);
        const int pix = slot >> 2, q = slot & 3;
        const int iy = pix / OC_I, ix = pix - iy * OC_I;
        const int gy = oy0 + iy - 1, gx = ox0 + ix - 1;
        const int cy = min(max(gy, 0), a.H - 1), cx = min(max(gx, 0), a.W - 1);
        if (tid + s * 256 < OC_I * OC_I * 4 && gy == cy && gx == cx) live |= 1u << s;
        soff[s] = (unsigned)((size_t)(cy * a.W + cx) * (a.blocked ? 16 : C) + q * 4);       // inside the sample (NHWC) / inside a block plane
    }
    const size_t plane = (size_t)a.H * a.W;
    auto chunk_base = [&](int c0) {               // first element of the sample's 16-channel chunk c0
        return a.blocked ? ((size_t)b * (C >> 4) + (c0 >> 4)) * plane * 16 : (size_t)b * plane * C + c0;
    };
    f32x4 pre[NSL];
    auto prefetch = [&](int c0) {
#pragma unroll
        for (int s = 0; s < NSL; ++s) {
#if defined(PW_ABL) && PW_ABL == 11     // ablation (tools/mb/pw_abl.hip, wrong results): no input loads
            pre[s] = (f32x4){(float)soff[s], 1.f, 2.f, 3.f};
#else
            pre[s] = *reinterpret_cast<const f32x4*>(a.src + chunk_base(c0) + soff[s]);
#endif
        }
    };
    prefetch(0);                                  // the first chunk's quads fly while the GroupNorm scale / shift are derived
    // (second source: C1 = 0, never read; a literal nullptr there crashes hipcc 7.2's inliner)
    gn_prologue_lds(a.gn_tot, C, a.gn_bs, a.gn_tot, 0, 1, a.stat_rep, a.gn_gamma, a.gn_beta, a.gn_eps, 1.0 / ((double)a.H * a.W * (C / GN_GROUPS_C)), b, 1.0f, gnp, tid, 256);
    for (int c0 = 0; c0 < C; c0 += 16) {
        __syncthreads();                          // the previous chunk's taps are done with the tile
#pragma unroll
        for (int s = 0; s < NSL; ++s) {
            const int slot = tid + s * 256;
            if (slot < OC_I * OC_I * 4) {
                const int q = slot & 3;
                const f32x4 sc = *reinterpret_cast<const f32x4*>(gnp + c0 + q * 4);
                const f32x4 sh = *reinterpret_cast<const f32x4*>(gnp + C + c0 + q * 4);
                f32x4 v = pre[s] * sc + sh;
#if !(defined(PW_ABL) && PW_ABL == 12)  // ablation: no SiLU
                v.x = silu_pw(v.x); v.y = silu_pw(v.y); v.z = silu_pw(v.z); v.w = silu_pw(v.w);
#endif
                if (!((live >> s) & 1u)) v = (f32x4){0.f, 0.f, 0.f, 0.f};      // the conv's zero padding
                *reinterpret_cast<f32x4*>(&tile[(slot >> 2) * OC_PS + q * 4]) = v;
            }
        }
        if (c0 + 16 < C) prefetch(c0 + 16);
        __syncthreads();
#if defined(PW_ABL) && PW_ABL == 13     // ablation: no taps
        acc[0] += tile[(ty * OC_I + tx) * OC_PS];
#else
#pragma unroll
        for (int tap = 0; tap < 9; ++tap) {
            const int dy = tap / 3, dx = tap - dy * 3;
            const float* px = &tile[((ty + dy) * OC_I + tx + dx) * OC_PS];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const f32x4 v = *reinterpret_cast<const f32x4*>(px + q * 4);
                if constexpr (IC > 0) {
#pragma unroll
                    for (int oc = 0; oc < IC; ++oc) {
                        // uniform address: scalar loads, the weights are SGPR operands (no LDS read, no register)
                        const f32x4 wv = *reinterpret_cast<const f32x4*>(wglob + (((oc * 9 + tap) * (C >> 4)) << 4) + c0 + q * 4);
                        acc[oc] = __builtin_fmaf(v.x, wv.x, __builtin_fmaf(v.y, wv.y, __builtin_fmaf(v.z, wv.z, __builtin_fmaf(v.w, wv.w, acc[oc]))));
                    }
                } else {
                    for (int oc = 0; oc < ic; ++oc) {
                        const f32x4 wv = *reinterpret_cast<const f32x4*>(&wl[(oc * 9 + tap) * C + c0 + q * 4]);
                        acc[oc] += v.x * wv.x + v.y * wv.y + v.z * wv.z + v.w * wv.w;
                    }
                }
            }
        }
#endif
    }
    const int oy = oy0 + ty, ox = ox0 + tx;
    if (oy >= a.H || ox >= a.W) return;
#pragma unroll
    for (int oc = 0; oc < (IC ? IC : 4); ++oc) {
        if (oc >= ic) break;
        const size_t o = (((size_t)b * ic + oc) * a.H + oy) * a.W + ox;
        float eps = acc[oc] + a.bias[oc];
        if (a.eps_out) a.eps_out[o] = eps;
#if MIDD_OUT_SLOTS
        if (a.x) {
            // The update of the two kernels above with the record's coefficients, every contraction written out as hipcc makes it
            // there (profiles/step_noise_isa.txt, profiles/slots_isa.txt): v_fma_f32 (-c2, eps, x), v_mul_f32 by c1, one fused
            // multiply-add for the noise term, clamp.  A uniform table must give mi_denoise's bits (tests/test_gpu_slots.py, G1).
#pragma clang fp contract(off)
            if (a.clamp_eps) eps = fminf(fmaxf(eps, -5.0f), 5.0f);
            float xn = rec.c1 * __builtin_fmaf(-rec.c2, eps, a.x[o]);
            if (rec.active & SLOT_NOISE) {        // (t > 0 and the call has a noise term)
                if (a.seeded) {
                    // the slot is a virtual sample: the element index of out_conv_seeded_kernel below with the record's frame -- (W, H*W, 0)
                    // for a whole image, a tile's place in its image otherwise -- and the record's member word (scalar arithmetic)
                    const uint32_t elem = (uint32_t)oc * rec.plane + (uint32_t)oy * rec.pitch + (uint32_t)ox + rec.origin;
                    xn = __builtin_fmaf(rec.c3, step_noise_value(a.seed, (long long)rec.image, (int)rec.iter, elem, rec.member), xn);
                } else if (a.noise) {
                    xn = __builtin_fmaf(rec.c3, a.noise[o], xn);
                }
            }
            a.x[o] = fminf(fmaxf(xn, 0.0f), 1.0f);
        }
#elif MIDD_OUT_DDIM
        if (a.x) {
            // THE DDIM UPDATE (include/midd.h), fp32, every operation rounded on its own: no contraction in this block, so the
            // seeded and the tensor form round s * noise alike and tests/ddim_update_reference.py restates it bit for bit.
#pragma clang fp contract(off)
            if (a.clamp_eps) eps = fminf(fmaxf(eps, -5.0f), 5.0f);
            const float x = a.x[o];
            float x0 = k.k0 * (x - k.k1 * eps);
            if (k.clip_x0) {
                const float c = fminf(fmaxf(x0, 0.0f), 1.0f);
                if (c != x0) eps = (x - k.r0 * c) * k.r1;      // eps re-derived: x_prev stays on the trajectory towards the clipped image
                x0 = c;
            }
            float xn = k.a * x0 + k.b * eps;
            if (k.s > 0.0f) {                                  // (launch-uniform: nothing is drawn or read at s == 0)
                if constexpr (MIDD_OUT_SEEDED) {
                    // the virtual sample and the element index of out_conv_seeded_kernel below, word for word
                    const uint32_t v = (uint32_t)a.v0 + (uint32_t)b, vi = v / (uint32_t)a.members;
                    uint32_t pitch = (uint32_t)a.W, plane = (uint32_t)a.H * (uint32_t)a.W, origin = 0, member = v - vi * (uint32_t)a.members;
                    if (a.tiles_x) {
                        const int ky = (int)member / a.tiles_x, kx = (int)member - ky * a.tiles_x;
                        pitch = (uint32_t)a.img_W; plane = (uint32_t)a.img_H * (uint32_t)a.img_W;
                        origin = (uint32_t)tile_origin(ky, a.img_H, a.H, a.tiles_y) * pitch + (uint32_t)tile_origin(kx, a.img_W, a.W, a.tiles_x);
                        member = 0;
                    }
                    const uint32_t elem = (uint32_t)oc * plane + (uint32_t)oy * pitch + (uint32_t)ox + origin;
                    xn = xn + k.s * step_noise_value(a.seed, a.sample_offset + vi, a.iter, elem, a.member_offset + member);
                } else {
                    if (a.noise) xn = xn + k.s * a.noise[o];
                }
            }
            if (k.last) xn = fminf(fmaxf(xn, 0.0f), 1.0f);      // the call returns an image in [0, 1]; intermediate x is not clamped
            a.x[o] = xn;
        }
#elif MIDD_OUT_DPM
        if (a.x) {
            // THE DPMPP2M UPDATE (include/midd.h), fp32, every operation rounded on its own: the DDIM update at eta = 0, word for
            // word, then the multistep term on the clipped predictions.  tests/dpm_update_reference.py restates it bit for bit.
#pragma clang fp contract(off)
            if (a.clamp_eps) eps = fminf(fmaxf(eps, -5.0f), 5.0f);
            const float x = a.x[o];
            float x0 = k.k0 * (x - k.k1 * eps);
            if (k.clip_x0) {
                const float c = fminf(fmaxf(x0, 0.0f), 1.0f);
                if (c != x0) eps = (x - k.r0 * c) * k.r1;      // eps re-derived: x_prev stays on the trajectory towards the clipped image
                x0 = c;
            }
            float xn = k.a * x0 + k.b * eps;
            if (k.g != 0.0f) xn = xn + k.g * (x0 - x0_prev[o]);      // (launch-uniform: the history is not read at g == 0; this
                                                                     //  thread's own element, read before it is written below)
            if (k.last) xn = fminf(fmaxf(xn, 0.0f), 1.0f);      // the call returns an image in [0, 1]; intermediate x is not clamped
            x0_out[o] = x0;
            a.x[o] = xn;
        }
#elif MIDD_OUT_SLOTS_RULE
        if (a.x) {
            // THE DDIM UPDATE / THE DPMPP2M UPDATE (include/midd.h) of the two blocks above, word for word, every scalar from the slot's
            // record: fp32, every operation rounded on its own.  A uniform table must give mi_denoise_rule's / mi_denoise_dpm's bits
            // (tests/test_gpu_slots_rule.py).
#pragma clang fp contract(off)
            if (a.clamp_eps) eps = fminf(fmaxf(eps, -5.0f), 5.0f);
            const float x = a.x[o];
            float x0 = rec.k0 * (x - rec.k1 * eps);
            if (clip_x0) {
                const float c = fminf(fmaxf(x0, 0.0f), 1.0f);
                if (c != x0) eps = (x - rec.r0 * c) * rec.r1;  // eps re-derived: x_prev stays on the trajectory towards the clipped image
                x0 = c;
            }
            float xn = rec.a * x0 + rec.b * eps;
            if (rec.s > 0.0f && (rec.active & SLOT_NOISE)) {   // (uniform in the workgroup: nothing is drawn or read otherwise)
                if (a.seeded) {
                    // the draw of out_conv_slots_kernel above: the record's frame, member word, image and iteration
                    const uint32_t elem = (uint32_t)oc * rec.plane + (uint32_t)oy * rec.pitch + (uint32_t)ox + rec.origin;
                    xn = xn + rec.s * step_noise_value(a.seed, (long long)rec.image, (int)rec.iter, elem, rec.member);
                } else if (a.noise) {
                    xn = xn + rec.s * a.noise[o];
                }
            }
            if (rec.active & SLOT_HIST) xn = xn + rec.g * (x0 - x0_hist[o]);      // (g != 0; this thread's own element, read before it is
                                                                                  //  written below)
            if (rec.active & SLOT_LAST) xn = fminf(fmaxf(xn, 0.0f), 1.0f);        // the slot's list ends: an image in [0, 1]
            if (x0_hist) x0_hist[o] = x0;
            a.x[o] = xn;
        }
#else
        if (a.x) {
            const float c1 = a.c1, c2 = a.c2, c3 = a.c3;
            const float* noise = a.noise;
            // x <- clamp( (1/sqrt(alpha)) * (x - ((1-alpha)/sqrt(1-alpha_hat)) * eps) [+ sqrt(beta)*noise], 0, 1 )
            // evaluated with the reference's operation order and no fused multiply-add.
            if (a.clamp_eps) eps = fminf(fmaxf(eps, -5.0f), 5.0f);
            float xn = __fmul_rn(c1, __fsub_rn(a.x[o], __fmul_rn(c2, eps)));
            if constexpr (MIDD_OUT_SEEDED) {
                // virtual sample -> (image, member): b is uniform in the workgroup, so this is one scalar division per workgroup
                const uint32_t v = (uint32_t)a.v0 + (uint32_t)b, vi = v / (uint32_t)a.members;
                // element index oc * plane + y * pitch + x + origin: inside the sample's [ic,H,W] block (W, H*W, 0), or -- a tile
                // of mi_denoise_tiled -- inside the whole image at the tile's origin (the host refuses ic * plane >= 2^32).
                // Uniform in the workgroup: scalar arithmetic
                uint32_t pitch = (uint32_t)a.W, plane = (uint32_t)a.H * (uint32_t)a.W, origin = 0, member = v - vi * (uint32_t)a.members;
                if (a.tiles_x) {
                    const int ky = (int)member / a.tiles_x, kx = (int)member - ky * a.tiles_x;
                    pitch = (uint32_t)a.img_W; plane = (uint32_t)a.img_H * (uint32_t)a.img_W;
                    origin = (uint32_t)tile_origin(ky, a.img_H, a.H, a.tiles_y) * pitch + (uint32_t)tile_origin(kx, a.img_W, a.W, a.tiles_x);
                    member = 0;
                }
                const uint32_t elem = (uint32_t)oc * plane + (uint32_t)oy * pitch + (uint32_t)ox + origin;
                // The term is added as ONE fused multiply-add, because that is what the unseeded twin below compiles to (hipcc's
                // __fmul_rn / __fadd_rn are the plain operators and it contracts them: v_fmac_f32, profiles/step_noise_isa.txt) and a
                // seeded run must replay through the noise tensor bit for bit.  Left to the compiler, this side's contraction
                // depends on the code around it (with the division above it became v_pk_mul_f32 + v_add_f32).
                xn = __builtin_fmaf(c3, step_noise_value(a.seed, a.sample_offset + vi, a.iter, elem, a.member_offset + member), xn);
            } else {
                if (noise) xn = __fadd_rn(xn, __fmul_rn(c3, noise[o]));
            }
            a.x[o] = fminf(fmaxf(xn, 0.0f), 1.0f);
        }
#endif
    }
}
