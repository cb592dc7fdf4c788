// Topology (the module lists and state-dict keys of the network), weight repacking into the kernels' operand orders, and
// the timestep table: everything mi_unet_finalize uploads.
#include "midd_host.h"

using namespace midd;

static bool is_attn_level(const mi_unet_cfg& c, int i) {
    for (int k = 0; k < c.num_attention_levels; ++k) if (c.attention_levels[k] == i) return true;
    return false;
}

static void expect(mi_plan* p, const std::string& name, std::vector<int64_t> shape) {
    p->expected.push_back(name);
    p->expected_shape[name] = std::move(shape);
}
static void expect_conv(mi_plan* p, const std::string& n, int cin, int cout, int k) {
    expect(p, n + ".weight", {cout, cin, k, k}); expect(p, n + ".bias", {cout});
}
static void expect_vec2(mi_plan* p, const std::string& n, int c) { expect(p, n + ".weight", {c}); expect(p, n + ".bias", {c}); }
static void expect_linear(mi_plan* p, const std::string& n, int cin, int cout) {
    expect(p, n + ".weight", {cout, cin}); expect(p, n + ".bias", {cout});
}

static void expect_mod(mi_plan* p, const Mod& m) {
    const int te = p->cfg.time_emb_dim;
    switch (m.kind) {
        case MOD_RB:
            expect_linear(p, m.name + ".time_mlp.1", te, m.out_c);
            expect_vec2(p, m.name + ".block1.0", m.in_c);
            expect_conv(p, m.name + ".block1.2", m.in_c, m.out_c, 3);
            expect_vec2(p, m.name + ".block2.0", m.out_c);
            expect_conv(p, m.name + ".block2.3", m.out_c, m.out_c, 3);
            if (m.in_c != m.out_c) expect_conv(p, m.name + ".res_conv", m.in_c, m.out_c, 1);
            break;
        case MOD_ATTN:
            expect_vec2(p, m.name + ".norm", m.in_c);
            expect_conv(p, m.name + ".qkv", m.in_c, 3 * m.in_c, 1);
            expect_conv(p, m.name + ".proj", m.in_c, m.in_c, 1);
            break;
        case MOD_DOWN: expect_conv(p, m.name, m.in_c, m.out_c, 3); break;
        case MOD_UP:
            expect(p, m.name + ".weight", {m.in_c, m.out_c, 4, 4});
            expect(p, m.name + ".bias", {m.out_c});
            break;
    }
}

// Mirrors the module lists built by UNetDiffusion.__init__ (DDIMModel.py:182-211; cddpm
// bookkeeping cddpmModels.py:191-221).
int midd::build_topology(mi_plan* p) {
    const mi_unet_cfg& c = p->cfg;
    const int mc = c.model_channels, nres = c.num_levels;
    int ch = mc;
    std::vector<int> down_channels;
    auto idx_name = [](const char* pre, size_t i) { return std::string(pre) + "." + std::to_string(i); };
    for (int i = 0; i < nres; ++i) {
        const int out_ch = mc * c.channel_mult[i];
        for (int r = 0; r < c.num_res_blocks; ++r) {
            p->downs.push_back(Mod{MOD_RB, idx_name("downs", p->downs.size()), ch, out_ch});
            ch = out_ch; down_channels.push_back(ch);
            if (is_attn_level(c, i)) {
                p->downs.push_back(Mod{MOD_ATTN, idx_name("downs", p->downs.size()), ch, ch});
                down_channels.push_back(ch);
            }
        }
        if (i != nres - 1) {
            p->downs.push_back(Mod{MOD_DOWN, idx_name("downs", p->downs.size()), ch, ch});
            down_channels.push_back(ch);
        }
    }
    p->mid.push_back(Mod{MOD_RB, "mid_block1", ch, ch});
    p->mid.push_back(Mod{MOD_ATTN, "mid_attn", ch, ch});
    p->mid.push_back(Mod{MOD_RB, "mid_block2", ch, ch});
    for (int i = nres - 1; i >= 0; --i) {
        const int out_ch = mc * c.channel_mult[i];
        for (int j = 0; j < c.num_res_blocks + 1; ++j) {
            int in_ch;
            if (c.variant == MI_VARIANT_DDIM) in_ch = ch + ch;
            else {
                if (down_channels.empty()) return fail(MI_EINVAL, "cddpm topology: skip stack underflow");
                in_ch = ch + down_channels.back(); down_channels.pop_back();
            }
            p->ups.push_back(Mod{MOD_RB, idx_name("ups", p->ups.size()), in_ch, out_ch});
            ch = out_ch;
            if (is_attn_level(c, i) && (c.variant == MI_VARIANT_DDIM || j == 0))
                p->ups.push_back(Mod{MOD_ATTN, idx_name("ups", p->ups.size()), ch, ch});
        }
        if (i != 0) p->ups.push_back(Mod{MOD_UP, idx_name("ups", p->ups.size()), ch, ch});
    }
    p->final_c = ch;
    p->levels = nres;

    int col = 0;
    auto assign_cols = [&](std::vector<Mod>& v) { for (Mod& m : v) if (m.kind == MOD_RB) { m.temb_col = col; col += m.out_c; } };
    assign_cols(p->downs); assign_cols(p->mid); assign_cols(p->ups);
    p->temb_cols = col;

    expect_linear(p, "time_mlp.1", mc, c.time_emb_dim);
    expect_linear(p, "time_mlp.3", c.time_emb_dim, c.time_emb_dim);
    expect_conv(p, "in_conv", 2 * c.in_channels, mc, 3);
    for (const Mod& m : p->downs) expect_mod(p, m);
    for (const Mod& m : p->mid) expect_mod(p, m);
    for (const Mod& m : p->ups) expect_mod(p, m);
    expect_vec2(p, "out_conv.0", p->final_c);
    expect_conv(p, "out_conv.2", p->final_c, c.in_channels, 3);
    return MI_OK;
}

// ------------------------------------------------------------------------------ weight packing
struct Packer {
    std::vector<float> buf;
    size_t put(const float* p, size_t n) {               // 64-float (256 B) aligned
        size_t off = (buf.size() + 63) & ~(size_t)63;
        buf.resize(off + n);
        memcpy(buf.data() + off, p, n * sizeof(float));
        return off;
    }
    size_t put(const std::vector<float>& v) { return put(v.data(), v.size()); }
};

// torch Conv2d weight [Cout][Cin][KS][KS]  ->  [Cin/16][KS*KS][Cout/16][lane 64][4]
// lane = kq*16 + n holds W[cout = 16*tile + n][cin = 16*chunk + 4*kq + j][tap] in element j:
// the A-operand fragment order of conv_mfma_f32.hip.
static std::vector<float> pack_conv_f32(const float* w, int Cout, int Cin, int KS) {
    const int taps = KS * KS, nch = Cin / 16, ntile = Cout / 16;
    std::vector<float> out((size_t)nch * taps * ntile * 256);
    for (int c = 0; c < nch; ++c)
        for (int t = 0; t < taps; ++t)
            for (int nt = 0; nt < ntile; ++nt)
                for (int lane = 0; lane < 64; ++lane) {
                    const int n = lane & 15, kq = lane >> 4;
                    for (int j = 0; j < 4; ++j) {
                        const int co = nt * 16 + n, ci = c * 16 + kq * 4 + j;
                        out[((((size_t)c * taps + t) * ntile + nt) * 64 + lane) * 4 + j] =
                            w[((size_t)co * Cin + ci) * taps + t];
                    }
                }
    return out;
}

// Split-fp16 packing for conv_mfma_f16x3.hip:  [step][Cout/16][hi|lo][lane 64][8 fp16]  (planes == 2; planes == 1, compute
// "f16": the hi plane alone, [step][Cout/16][lane 64][8 fp16] -- fp16(w') of the same w').
// Steps walk 32 input channels (blocks 2c, 2c+1) per tap; a trailing single block pairs two
// taps per step.  lane = kq*16 + n; element j is W[16*tile+n][cin][tap] with
//   full chunk : cin = 16*(2c + (kq>>1)) + 8*(kq&1) + j, tap = step's tap
//   half chunk : cin = 16*(2c) + 8*(kq&1) + j,           tap = 2*hs + (kq>>1)  (zero when >= taps)
//   16-channel chunks of a 3x3 (cb == 1): the pair walk of conv16_pair_walk (midd_internal.h), spelled out below
// w' = w * 2^k (k per layer, max|w'| in [2^13,2^14)); hi = fp16(w'), lo = fp16(w' - hi).
// *out_scale = 2^-k / ACT_PRESCALE.  Returned as raw 32-bit words (two fp16 each).
static const float SILU_WEIGHT_FACTOR_H = -0.6931471805599453f;     // == SILU_WEIGHT_FACTOR (f16x3_common.h): see conv_mfma_f16x3.hip, transform
static std::vector<float> pack_conv_f16x3(const float* w_in, int Cout, int Cin, int KS, float* out_scale, int planes, float wmul = 1.0f, int cb = 0) {
    if (cb == 0) cb = conv16_cb(KS);                     // blocks per K chunk: the K order of the steps (midd_internal.h)
    // wmul: constant folded into the weights (fp32 product, rounded once): -ln 2 for the convolutions behind GroupNorm + SiLU,
    // whose operand the kernel forms as -16 log2(e) silu(y)
    std::vector<float> wm;
    const float* w = w_in;
    if (wmul != 1.0f) {
        wm.resize((size_t)Cout * Cin * KS * KS);
        for (size_t i = 0; i < wm.size(); ++i) wm[i] = w_in[i] * wmul;
        w = wm.data();
    }
    const int taps = KS * KS, nblk = Cin / 16, ntile = Cout / 16;
    const int steps = conv16_num_steps(Cin, taps, cb);
    float wmax = 0.f;
    for (size_t i = 0; i < (size_t)Cout * Cin * taps; ++i) wmax = std::fmax(wmax, std::fabs(w[i]));
    int e = 0;
    if (wmax > 0.f) (void)std::frexp(wmax, &e);          // wmax = m * 2^e, m in [0.5, 1)
    const int k = 14 - e;                                // max|w * 2^k| in [2^13, 2^14)
    const float wscale = std::ldexp(1.0f, k);
    *out_scale = std::ldexp(1.0f, -k) / ACT_PRESCALE_H;
    std::vector<_Float16> out((size_t)steps * ntile * planes * 64 * 8);
    int step = 0;
    auto emit = [&](int blk_of_kq0, int blk_of_kq2, int tap_of_kq0, int tap_of_kq2) {
        for (int nt = 0; nt < ntile; ++nt)
            for (int lane = 0; lane < 64; ++lane) {
                const int n = lane & 15, kq = lane >> 4;
                const int blk = (kq >> 1) ? blk_of_kq2 : blk_of_kq0;
                const int tap = (kq >> 1) ? tap_of_kq2 : tap_of_kq0;
                for (int j = 0; j < 8; ++j) {
                    float v = 0.f;
                    if (tap < taps) {
                        const int co = nt * 16 + n, ci = blk * 16 + 8 * (kq & 1) + j;
                        v = w[((size_t)co * Cin + ci) * taps + tap] * wscale;
                    }
                    const _Float16 hi = (_Float16)v;
                    const _Float16 lo = (_Float16)(v - (float)hi);
                    const size_t base = (((size_t)step * ntile + nt) * planes) * 64 * 8;
                    out[base + (size_t)lane * 8 + j] = hi;
                    if (planes == 2) out[base + 64 * 8 + (size_t)lane * 8 + j] = lo;
                }
            }
        ++step;
    };
    if (conv16_pair_walk(taps, cb)) {
        // pair walk: block c (even) in 4 steps, taps (0|1) (2|3) (4|5) (6|7); block c + 1 in 5: (tap 8 of block c | tap 0),
        // (1|2) (3|4) (5|6) (7|8).  An unpaired last block: 5 steps, the last one's upper half zero.
        for (int blk = 0; blk < nblk; blk += 2) {
            if (blk + 1 < nblk) {
                for (int hs = 0; hs < taps / 2; ++hs) emit(blk, blk, 2 * hs, 2 * hs + 1);
                emit(blk, blk + 1, taps - 1, 0);
                for (int hs = 0; hs < taps / 2; ++hs) emit(blk + 1, blk + 1, 2 * hs + 1, 2 * hs + 2);
            } else {
                for (int hs = 0; hs < (taps + 1) / 2; ++hs) emit(blk, blk, 2 * hs, 2 * hs + 1);
            }
        }
    } else if (cb == 1) {
        for (int blk = 0; blk < nblk; ++blk)
            for (int hs = 0; hs < (taps + 1) / 2; ++hs) emit(blk, blk, 2 * hs, 2 * hs + 1);
    } else {
        for (int c = 0; 2 * c < nblk; ++c) {
            if (2 * c + 1 < nblk) for (int t = 0; t < taps; ++t) emit(2 * c, 2 * c + 1, t, t);
            else for (int hs = 0; hs < (taps + 1) / 2; ++hs) emit(2 * c, 2 * c, 2 * hs, 2 * hs + 1);
        }
    }
    std::vector<float> words(out.size() / 2);
    memcpy(words.data(), out.data(), out.size() * sizeof(_Float16));
    return words;
}

// ConvTranspose2d(4,2,1) followed by the bilinear half-size resample (an exact 2x2 mean for
// align_corners=False) == one 3x3/s1/p1 conv with
//   W_eff[co][ci][d][e] = 1/4 * sum_{a,b in {0,1}} W[ci][co][a-2d+3][b-2e+3]   (indices within 0..3)
// (DDIMModel.py:211 + :241-242; identity checked in tests/test_oracle_vs_reference.py).
static std::vector<float> fold_convt(const float* w /*[Cin][Cout][4][4]*/, int Cin, int Cout) {
    std::vector<float> eff((size_t)Cout * Cin * 9, 0.f);
    for (int ci = 0; ci < Cin; ++ci)
        for (int co = 0; co < Cout; ++co)
            for (int d = 0; d < 3; ++d)
                for (int e = 0; e < 3; ++e) {
                    float acc = 0.f;
                    for (int a = 0; a < 2; ++a)
                        for (int b = 0; b < 2; ++b) {
                            const int ky = a - 2 * d + 3, kx = b - 2 * e + 3;
                            if (ky >= 0 && ky < 4 && kx >= 0 && kx < 4)
                                acc += w[(((size_t)ci * Cout + co) * 4 + ky) * 4 + kx];
                        }
                    eff[(((size_t)co * Cin + ci) * 3 + d) * 3 + e] = 0.25f * acc;
                }
    return eff;
}

static const HostWeight* getw(mi_plan* p, const std::string& k) {
    auto it = p->host.find(k);
    return (it != p->host.end() && it->second.loaded) ? &it->second : nullptr;
}

static inline float silu_h(float v) { return v / (1.0f + expf(-v)); }

static void linear_h(const float* w, const float* b, const float* x, float* y, int cin, int cout) {
    for (int o = 0; o < cout; ++o) {
        float acc = 0.f;
        const float* wr = w + (size_t)o * cin;
        for (int i = 0; i < cin; ++i) acc += wr[i] * x[i];
        y[o] = acc + b[o];
    }
}

// time_mlp of the network (DDIMModel.py:99-106,173-178) followed by each ResidualBlock's
// Linear(SiLU(t_emb)) (DDIMModel.py:111-114,130), for t = 0..rows-1 -> [rows][temb_cols] fp32.
static std::vector<float> build_time_table(mi_plan* p, int rows) {
    const int mc = p->cfg.model_channels, te = p->cfg.time_emb_dim, half = mc / 2;
    const HostWeight *w1 = getw(p, "time_mlp.1.weight"), *b1 = getw(p, "time_mlp.1.bias");
    const HostWeight *w3 = getw(p, "time_mlp.3.weight"), *b3 = getw(p, "time_mlp.3.bias");
    std::vector<float> freqs(half);
    // math.log(10000)/(half-1) is a Python double; arange(half) * -k promotes the scalar to fp32
    const float k = (float)(-(std::log(10000.0) / (double)(half - 1)));
    for (int j = 0; j < half; ++j) freqs[j] = expf((float)j * k);
    std::vector<float> table((size_t)rows * p->temb_cols);
    std::vector<float> e(mc), h1(te), temb(te), act(te);
    std::vector<const Mod*> rbs;
    for (auto* v : {&p->downs, &p->mid, &p->ups}) for (const Mod& m : *v) if (m.kind == MOD_RB) rbs.push_back(&m);
    for (int t = 0; t < rows; ++t) {
        for (int j = 0; j < half; ++j) {
            const float arg = (float)t * freqs[j];
            e[j] = sinf(arg); e[half + j] = cosf(arg);
        }
        linear_h(w1->data.data(), b1->data.data(), e.data(), h1.data(), mc, te);
        for (int i = 0; i < te; ++i) h1[i] = silu_h(h1[i]);
        linear_h(w3->data.data(), b3->data.data(), h1.data(), temb.data(), te, te);
        for (int i = 0; i < te; ++i) act[i] = silu_h(temb[i]);
        for (const Mod* m : rbs) {
            const HostWeight *w = getw(p, m->name + ".time_mlp.1.weight"), *b = getw(p, m->name + ".time_mlp.1.bias");
            linear_h(w->data.data(), b->data.data(), act.data(), &table[(size_t)t * p->temb_cols + m->temb_col], te, m->out_c);
        }
    }
    return table;
}

extern "C" int mi_unet_finalize(mi_plan* plan, int time_rows) {
    if (!plan) return fail(MI_EINVAL, "null plan");
    if (time_rows < 1) return fail(MI_EINVAL, "time_rows must be >= 1");
    std::lock_guard<std::mutex> lk(plan->mu);
    for (const std::string& k : plan->expected)
        if (!getw(plan, k)) return fail(MI_ESTATE, "missing key in state_dict: \"%s\"", k.c_str());

    Packer pk;
    const bool f16 = fp16_mfma(plan->cfg);               // either fp16-MFMA mode
    const int planes = operand_planes(plan->cfg);
    auto pack_conv = [&](const float* w, int Cout, int Cin, int KS, float* scale, bool behind_silu = false) {
        *scale = 1.0f;
        return f16 ? pack_conv_f16x3(w, Cout, Cin, KS, scale, planes, behind_silu ? SILU_WEIGHT_FACTOR_H : 1.0f) : pack_conv_f32(w, Cout, Cin, KS);
    };
    // second copy of a 3x3's weights in the wide-chunk K order (same values, same scale); the planner picks per launch
    auto pack_wide = [&](const float* w, int Cout, int Cin, bool behind_silu, const std::vector<float>* tail = nullptr) -> size_t {
        if (!packs_wide_copy(plan->cfg, Cin)) return (size_t)-1;
        float scale;
        std::vector<float> v = pack_conv_f16x3(w, Cout, Cin, 3, &scale, planes, behind_silu ? SILU_WEIGHT_FACTOR_H : 1.0f, 2);
        if (tail) v.insert(v.end(), tail->begin(), tail->end());
        return pk.put(v);
    };
    auto W = [&](const std::string& k) { return getw(plan, k)->data.data(); };
    auto put_raw = [&](const std::string& k) { return pk.put(getw(plan, k)->data); };
    auto pack_mod = [&](Mod& m) {
        switch (m.kind) {
            case MOD_RB:
                m.g1 = put_raw(m.name + ".block1.0.weight"); m.be1 = put_raw(m.name + ".block1.0.bias");
                m.w1 = pk.put(pack_conv(W(m.name + ".block1.2.weight"), m.out_c, m.in_c, 3, &m.s1, true)); m.b1 = put_raw(m.name + ".block1.2.bias");
                m.w1x = pack_wide(W(m.name + ".block1.2.weight"), m.out_c, m.in_c, true);
                m.g2 = put_raw(m.name + ".block2.0.weight"); m.be2 = put_raw(m.name + ".block2.0.bias");
                {
                    std::vector<float> w2p = pack_conv(W(m.name + ".block2.3.weight"), m.out_c, m.out_c, 3, &m.s2, true);
                    m.b2 = put_raw(m.name + ".block2.3.bias");
                    if (m.in_c == m.out_c) m.w2x = pack_wide(W(m.name + ".block2.3.weight"), m.out_c, m.out_c, true);
                    if (m.in_c != m.out_c) {
                        const std::vector<float> wrp = pack_conv(W(m.name + ".res_conv.weight"), m.out_c, m.in_c, 1, &m.sr);
                        m.wr = pk.put(wrp); m.br = put_raw(m.name + ".res_conv.bias");
                        if (f16) {
                            m.w2x = pack_wide(W(m.name + ".block2.3.weight"), m.out_c, m.out_c, true, &wrp);
                            // res_conv folded into conv2 (conv_mfma_f16x3.hip: res phase): its K steps (32 channels each, same
                            // per-step layout) follow the 3x3 steps; one bias vector
                            w2p.insert(w2p.end(), wrp.begin(), wrp.end());
                            std::vector<float> bsum(m.out_c);
                            const float* b2 = W(m.name + ".block2.3.bias"); const float* br = W(m.name + ".res_conv.bias");
                            for (int i = 0; i < m.out_c; ++i) bsum[i] = b2[i] + br[i];
                            m.b2r = pk.put(bsum);
                        }
                    }
                    m.w2 = pk.put(w2p);
                }
                break;
            case MOD_ATTN:
                m.g1 = put_raw(m.name + ".norm.weight"); m.be1 = put_raw(m.name + ".norm.bias");
                m.wq = pk.put(pack_conv(W(m.name + ".qkv.weight"), 3 * m.in_c, m.in_c, 1, &m.sq)); m.bq = put_raw(m.name + ".qkv.bias");
                m.wp = pk.put(pack_conv(W(m.name + ".proj.weight"), m.in_c, m.in_c, 1, &m.sp)); m.bp = put_raw(m.name + ".proj.bias");
                break;
            case MOD_DOWN:
                m.wc = pk.put(pack_conv(W(m.name + ".weight"), m.out_c, m.in_c, 3, &m.sc)); m.bc = put_raw(m.name + ".bias");
                break;
            case MOD_UP: {
                const float* w = W(m.name + ".weight");
                std::vector<float> eff = fold_convt(w, m.in_c, m.out_c);
                m.wc = pk.put(pack_conv(eff.data(), m.out_c, m.in_c, 3, &m.sc)); m.bc = put_raw(m.name + ".bias");
                m.wcx = pack_wide(eff.data(), m.out_c, m.in_c, false);
                // raw layout [ky][kx][Cin][Cout] for the direct fallback kernel
                std::vector<float> raw((size_t)16 * m.in_c * m.out_c);
                for (int ci = 0; ci < m.in_c; ++ci) for (int co = 0; co < m.out_c; ++co)
                    for (int ky = 0; ky < 4; ++ky) for (int kx = 0; kx < 4; ++kx)
                        raw[(((size_t)(ky * 4 + kx)) * m.in_c + ci) * m.out_c + co] = w[(((size_t)ci * m.out_c + co) * 4 + ky) * 4 + kx];
                m.wt = pk.put(raw);
                break;
            }
        }
    };
    for (Mod& m : plan->downs) pack_mod(m);
    for (Mod& m : plan->mid) pack_mod(m);
    for (Mod& m : plan->ups) pack_mod(m);
    {   // in_conv [Cout][2ic][3][3] -> [tap][2ic][Cout]
        const int ci2 = 2 * plan->cfg.in_channels, co = plan->cfg.model_channels;
        const float* w = W("in_conv.weight");
        std::vector<float> t((size_t)9 * ci2 * co);
        for (int o = 0; o < co; ++o) for (int i = 0; i < ci2; ++i) for (int tap = 0; tap < 9; ++tap)
            t[((size_t)tap * ci2 + i) * co + o] = w[((size_t)o * ci2 + i) * 9 + tap];
        plan->w_in = pk.put(t); plan->b_in = put_raw("in_conv.bias");
    }
    {   // out_conv.2 [ic][C][3][3] -> [ic][tap][C]
        const int ic = plan->cfg.in_channels, C = plan->final_c;
        const float* w = W("out_conv.2.weight");
        std::vector<float> t((size_t)ic * 9 * C);
        for (int o = 0; o < ic; ++o) for (int c = 0; c < C; ++c) for (int tap = 0; tap < 9; ++tap)
            t[((size_t)o * 9 + tap) * C + c] = w[((size_t)o * C + c) * 9 + tap];
        plan->g_out = put_raw("out_conv.0.weight"); plan->be_out = put_raw("out_conv.0.bias");
        plan->w_out = pk.put(t); plan->b_out = put_raw("out_conv.2.bias");
    }
    std::vector<float> table = build_time_table(plan, time_rows);

    HIPCHK(hipGetDevice(&plan->device));
    // Programs cache per-layer values derived from the weights (Op::out_scale = 2^-k of the f16x3 packing): they are
    // rebuilt after every (re)finalize.  hipFree below synchronises the device, so nothing that still reads the old
    // buffers is in flight.
    plan->programs.clear();
    if (plan->wdev) { HIPCHK(hipFree(plan->wdev)); plan->wdev = nullptr; }
    if (plan->ttab) { HIPCHK(hipFree(plan->ttab)); plan->ttab = nullptr; }
    HIPCHK(hipMalloc((void**)&plan->wdev, pk.buf.size() * sizeof(float)));
    HIPCHK(hipMemcpy(plan->wdev, pk.buf.data(), pk.buf.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc((void**)&plan->ttab, table.size() * sizeof(float)));
    HIPCHK(hipMemcpy(plan->ttab, table.data(), table.size() * sizeof(float), hipMemcpyHostToDevice));
    plan->time_rows = time_rows;
    plan->finalized = true;
    return MI_OK;
}
