// Seeded step noise of the stochastic sampler (cddpmModels.py:297-302: x += sqrt(beta_t) * 0.5 * randn_like(x) for t > 0) as a
// counter-based generator: every value is a pure function of (seed, global sample index, iteration index, element index, member
// index), so it does not depend on the batch a sample is computed in, on the two-stream split, on the stream or on the GPU that
// holds the sample.  The member index separates the draws of an ensemble (mi_denoise_ensemble): member 0 is the single seeded run.
// The specification (include/midd.h; tests/step_noise_reference.py restates it in numpy):
//   Philox4x32-10 as in Random123: multipliers 0xD2511F53 / 0xCD9E8D57, key increments 0x9E3779B9 / 0xBB67AE85, ten rounds
//   counter  c0 = element index inside the sample's [C,H,W] block (C*H*W < 2^32), c1 = low word of the global sample index
//            (the IMAGE's: sample_offset + b), c2 = iteration index (position in t_list), c3 = member index (0 for
//            mi_denoise_seeded and mi_step_noise_fill; the ensemble calls number an image's draws 0, 1, 2, ...)
//            tiles of mi_denoise_tiled: c0 = the pixel's index in the WHOLE image, (c * H_img + y0 + y) * W_img + x0 + x
//   key      k0 = low word of the seed, k1 = high word
//   one call per element; outputs x0, x1 are used:
//   u1 = ((x0 >> 8) + 1) * 2^-24  in (0, 1]      u2 = (x1 >> 8) * 2^-24  in [0, 1)      (both exact in fp32)
//   z  = sqrtf(-2 * logf(u1)) * cospif(2 * u2)   accurate library functions, every product rounded on its own; |z| <= 5.77
// Used by out_conv_seeded_kernel (the fused sampler update) and step_noise_fill_kernel (replay / export), both in out_conv.hip:
// one function, so the two agree bit for bit.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace midd {

struct Philox4 { uint32_t x0, x1, x2, x3; };

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0;
        const uint32_t hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1;
        c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += W0; k1 += W1;
    }
    return Philox4{c0, c1, c2, c3};
}

// the standard normal z of (seed, sample, iteration, element, member), times 0.5: the value the `step_noise` tensors carry
__device__ __forceinline__ float step_noise_value(unsigned long long seed, long long sample, int iter, uint32_t elem, uint32_t member) {
    const Philox4 r = philox4x32_10(elem, (uint32_t)(unsigned long long)sample, (uint32_t)iter, member,
                                    (uint32_t)seed, (uint32_t)(seed >> 32));
    constexpr float TWO_M24 = 5.9604644775390625e-08f;
    const float u1 = __fmul_rn((float)((r.x0 >> 8) + 1u), TWO_M24);
    const float u2 = __fmul_rn((float)(r.x1 >> 8), TWO_M24);
    const float z = __fmul_rn(sqrtf(__fmul_rn(-2.0f, logf(u1))), cospif(__fmul_rn(2.0f, u2)));
    return __fmul_rn(0.5f, z);
}

// THE FORWARD NOISE (include/midd.h; diffusion_loss.hip): the standard normal z itself -- no 0.5 -- of (seed, sample, draw, element),
// 0 <= draw < 2^31.  The same generator with the counter words (element, sample, 0x80000000 | draw, 0): a sampler iteration index
// never has the top bit of c2 set, so no value here is a step-noise value of the same seed.  A sibling, not a refactoring:
// step_noise_value above and the kernels that call it are untouched.
__device__ __forceinline__ float forward_noise_value(unsigned long long seed, uint32_t sample, uint32_t draw, uint32_t elem) {
    const Philox4 r = philox4x32_10(elem, sample, 0x80000000u | draw, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
    constexpr float TWO_M24 = 5.9604644775390625e-08f;
    const float u1 = __fmul_rn((float)((r.x0 >> 8) + 1u), TWO_M24);
    const float u2 = __fmul_rn((float)(r.x1 >> 8), TWO_M24);
    return __fmul_rn(sqrtf(__fmul_rn(-2.0f, logf(u1))), cospif(__fmul_rn(2.0f, u2)));
}

}  // namespace midd
