/*
 * midd.h — C ABI of libmidd.so, the MI355X (gfx950) native implementation of the
 * reverse-diffusion sampler path.
 *
 * The reference has no FFI/operator interface for this path: its boundary is two Python
 * classes, UNetDiffusion / DiffusionDenoiser (/root/reference/Backend/DDIM/DDIMModel.py:169-289),
 * imported by name at /root/reference/Backend/run.py:13.  Every entry point below cites the
 * reference interface it replaces; the ctypes binding a maintainer adds on the reference
 * side is shown in INTEGRATION.md.
 *
 * Conventions
 *   - plain C: opaque handle, pointers and sizes only; no torch / C++ types.
 *   - every function returns 0 on success or a negative MI_E* code; the message is
 *     available from mi_last_error() (thread-local).  Nothing throws across the ABI.
 *   - image / workspace pointers are DEVICE pointers on the current HIP device; weight,
 *     schedule and timestep-list pointers are HOST pointers.
 *   - forward/denoise allocate nothing: the caller supplies the workspace (size from
 *     mi_workspace_bytes) and a stream (void* = hipStream_t, NULL = default stream).
 *     They are asynchronous with respect to the host; the caller synchronises.
 *   - a plan is immutable after mi_unet_finalize and may be shared by threads; concurrent
 *     calls must use distinct workspaces (run.py:85-91 calls the sampler from a worker thread).
 *   - images are fp32, contiguous [B, in_channels, H, W] exactly as the reference passes
 *     them (DDIMModel.py:219, :269); H and W must be multiples of 2^(levels-1) (8) -- mi_denoise_tiled lifts that for images.
 */
#ifndef MIDD_H
#define MIDD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MI_OK            0
#define MI_EINVAL       -1   /* bad argument / unsupported shape or topology */
#define MI_ESTATE       -2   /* call order (e.g. forward before finalize, missing weight) */
#define MI_EHIP         -3   /* a HIP runtime call or kernel launch failed */
#define MI_ENOMEM       -4   /* workspace too small */
#define MI_ERANGE       -5   /* mi_status: the last call met values outside what its arithmetic represents */

/* bits of the status word (mi_status) */
#define MI_STATUS_NONFINITE   1   /* NaN / Inf activations reached a GroupNorm statistic or a raw conv operand -- or FINITE ones
                                   * beyond the statistics range.  SUPPORTED ACTIVATION RANGE: the GroupNorm totals are fixed point
                                   * with range +-2^59 (csrc/stats_common.h), and a producer workgroup's fp32 partial sum of squares
                                   * of one channel of one sample that reaches 2^59 counts as not a number: the group is NaN in the
                                   * output and the call reports MI_ERANGE with this bit.  A workgroup covers between one tile (16 ..
                                   * 128 pixels) and one sample's whole map, so
                                   *   never reported:   rms of every channel of every activation map < 2^29.5 / sqrt(H * W) of that map
                                   *                     (2.4e7 at 24 x 40, 3.0e6 at 256 x 256, 1.5e6 at 512 x 512),
                                   *   always reported:  any |activation| >= 2^29.5 = 7.6e8,
                                   * and between the two it depends on the launch's tiles.  Below, partials under 2^-37 lose low bits
                                   * and nothing else.  fp32 torch has no such limit: the reference is finite and right until fp32
                                   * itself overflows (squares of 1.8e19). */
#define MI_STATUS_FP16_RANGE  2   /* fp16-MFMA modes (f16x3, f16): an attention operand (q, k, v) beyond +-4094 */

#define MI_MAX_LEVELS    8

#define MI_VARIANT_DDIM  0   /* Backend/DDIM/DDIMModel.py  */
#define MI_VARIANT_CDDPM 1   /* Backend/cddpm/cddpmModels.py */

/* arithmetic of the MFMA contractions (convolutions, attention) */
#define MI_COMPUTE_F32   0   /* fp32-input MFMA: bit-for-bit an fp32 fma chain */
#define MI_COMPUTE_F16X3 1   /* fp32 operands split into two fp16 halves, three fp16 MFMAs, fp32 accumulate
                                (~2^-21 relative per product; same parity gate) — about 5x the MFMA rate */
#define MI_COMPUTE_F16   2   /* every MFMA multiplicand rounded ONCE to fp16 (the hi half of the split above, same
                                prescales), one fp16 MFMA per product, fp32 accumulate; activations, statistics, softmax
                                sums and epilogues stay fp32.  NOT a parity mode: ~2^-11 relative per operand, judged
                                against the reference under autocast; same operand-range rule */
/* OR into compute_mode: results of a sample do not depend on the batch it is computed in, bit for bit
 * (denoise(x[:k]) == denoise(x)[:k]; SURVEY.md section 8e "sharded == single-GPU").  Tiles, persistent workgroups per
 * sample, chunk width and the attention key split are then chosen as the default plan of a 4-sample sub-batch chooses
 * them -- the grouping of the fp32 partial sums behind the GroupNorm statistics no longer varies with the batch.
 * Free at batch 8 (the plan is the default one), -6 % at batch 32, +12 % on the latency of a single image. */
#define MI_COMPUTE_BATCH_INVARIANT 0x100

/* sampler flags for mi_denoise */
#define MI_CLAMP_EPS     1   /* clamp(eps,-5,5) before the update: DDIMModel.py:278 (absent in cddpm) */
#define MI_NO_SPLIT      2   /* run the batch as ONE program on the caller's stream (default: two half-batches on two streams);
                                same results to rounding (per-program batch changes the tiles), used by bench.py's roofline leg */

typedef struct mi_plan mi_plan;

/* Constructor arguments of UNetDiffusion.__init__ (DDIMModel.py:169-170). */
typedef struct mi_unet_cfg {
    int32_t in_channels;                         /* 1 */
    int32_t model_channels;                      /* 48; must be a multiple of 16 */
    int32_t num_levels;                          /* len(channel_mult) = 4 */
    int32_t channel_mult[MI_MAX_LEVELS];         /* (1,2,3,4) */
    int32_t num_res_blocks;                      /* 2 */
    int32_t num_attention_levels;                /* len(attention_resolutions) = 1 */
    int32_t attention_levels[MI_MAX_LEVELS];     /* (3,) — level indices */
    int32_t time_emb_dim;                        /* 192 */
    int32_t variant;                             /* MI_VARIANT_* */
    int32_t compute_mode;                        /* MI_COMPUTE_* (not a reference argument) */
} mi_unet_cfg;

/* Replaces UNetDiffusion.__init__ (DDIMModel.py:169-217): derives the module lists
 * (downs / mid / ups) and the expected state-dict entries. */
int mi_unet_plan_create(const mi_unet_cfg* cfg, mi_plan** out);

/* Replaces model.load_state_dict(ckpt['model_state_dict']) (run.py:37-39): called once per
 * state-dict entry with the reference's key name (e.g. "downs.3.block1.2.weight",
 * "ups.6.weight" [Cin,Cout,4,4]).  `data` is a HOST pointer to contiguous fp32. */
int mi_unet_load_weights(mi_plan* plan, const char* key, const float* data,
                         const int64_t* shape, int ndim);

/* Number of state-dict entries the plan expects / the i-th expected key (for the host
 * shim's strict-load check). */
int mi_unet_num_weights(const mi_plan* plan);
const char* mi_unet_weight_name(const mi_plan* plan, int index);

/* Repacks all weights into kernel layouts on the device (MFMA fragment order, folded
 * ConvTranspose+resample 3x3 — DDIMModel.py:211,241-242), and precomputes the timestep
 * table: time_mlp (DDIMModel.py:99-106,173-178) followed by every ResidualBlock's
 * Linear(SiLU(.)) (DDIMModel.py:111-114,130) for t in [0, time_rows).
 * May be called again after further mi_unet_load_weights calls (re-uploads). */
int mi_unet_finalize(mi_plan* plan, int time_rows);

/* Bytes of device workspace one forward/denoise call needs at this shape. */
size_t mi_workspace_bytes(mi_plan* plan, int B, int H, int W);

/* Replaces UNetDiffusion.forward(x, condition, t) (DDIMModel.py:219-248).
 * x, condition: device fp32 [B,in_channels,H,W]; t: HOST int32[B] (the reference takes an
 * int64 tensor; the sampler always passes B equal values, DDIMModel.py:275);
 * eps: device fp32 [B,in_channels,H,W]. */
int mi_unet_forward(mi_plan* plan, const float* x, const float* condition, const int32_t* t,
                    float* eps, int B, int H, int W,
                    void* workspace, size_t workspace_bytes, void* stream);

/* Replaces DiffusionDenoiser.denoise(noisy_img, inference_steps) (DDIMModel.py:268-289; cddpm:
 * cddpmModels.py:281-308).  The iteration list and the schedule tables are passed in by the
 * host shim, which computes them exactly as the reference does (DDIMModel.py:255-257,272-274).
 *   noisy      device fp32 [B,C,H,W]; never written (DDIMModel.py:271 clones it)
 *   x_out      device fp32 [B,C,H,W]; receives x after the last iteration
 *   t_list     HOST int32[n_iters] timesteps in execution order (each < noise_steps <= time_rows)
 *   beta/alpha/alpha_hat  HOST fp32[noise_steps]
 *   step_noise device fp32 [n_iters,B,C,H,W] or NULL: the already 0.5-scaled Gaussian noise of
 *              the cddpm variant (cddpmModels.py:297-302); entry i is ignored when t_list[i]==0
 *   flags      MI_CLAMP_EPS for the DDIM variant; MI_NO_SPLIT */
int mi_denoise(mi_plan* plan, const float* noisy, float* x_out, int B, int H, int W,
               const int32_t* t_list, int n_iters,
               const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
               const float* step_noise, int flags,
               void* workspace, size_t workspace_bytes, void* stream);

/* mi_denoise for the cddpm variant with the step noise drawn ON THE DEVICE, inside the fused update, from a seeded counter-based
 * generator (the reference draws torch.randn_like(x) per iteration, cddpmModels.py:297-302; its generator stream is not
 * reproduced).  No noise tensor exists.  Same arguments as mi_denoise without `step_noise`, plus
 *   seed           any 64-bit value
 *   sample_offset  global index of sample 0 of this call (>= 0): a caller that splits a batch over calls, streams or GPUs passes
 *                  each part its offset and gets the noise the whole batch would have got, bit for bit.  The two-stream split
 *                  inside the call does the same (sub-batch h of `parts` passes sample_offset + h * B / parts).
 * Every value is a pure function of (seed, global sample index, iteration index i, element index, member index): it does not
 * depend on B, on MI_NO_SPLIT, on the stream or on the device.  THE SPECIFICATION (fixed):
 *   Philox4x32-10 as in Random123: multipliers 0xD2511F53, 0xCD9E8D57; key increments 0x9E3779B9, 0xBB67AE85; ten rounds
 *   counter  c0 = element index inside the sample's [C,H,W] block (C*H*W < 2^32, else MI_EINVAL), c1 = low 32 bits of
 *            sample_offset + b (the global IMAGE index), c2 = i (position in t_list), c3 = member index; 0 for mi_denoise_seeded
 *            (mi_denoise_ensemble numbers the draws of one image member_offset, member_offset + 1, ...);
 *            in general c0 = c * plane + y * pitch + x + origin with (pitch, plane, origin) = (W, H*W, 0) for every call above;
 *            a TILE of mi_denoise_tiled at (y0, x0) of an image [C,H_img,W_img] uses (W_img, H_img*W_img, y0*W_img + x0), i.e.
 *            c0 = (c*H_img + y0 + y)*W_img + x0 + x, the pixel's index in the WHOLE image (C*H_img*W_img < 2^32), c3 = 0;
 *            key  k0, k1 = low, high word of seed
 *   one Philox call per element, outputs x0 and x1 used:
 *   u1 = ((x0 >> 8) + 1) * 2^-24 in (0, 1],   u2 = (x1 >> 8) * 2^-24 in [0, 1)   (exact in fp32)
 *   z  = sqrtf(-2 * logf(u1)) * cospif(2 * u2)   (accurate fp32 library functions, each product rounded once; |z| <= 5.77)
 *   x += sqrt(beta_t) * (0.5 * z)   for t_list[i] > 0, where mi_denoise adds sqrt(beta_t) * step_noise[i]; nothing is drawn at t == 0
 * With the DDIM variant's flags the call works too and simply adds the term; the host shims never seed that variant. */
int mi_denoise_seeded(mi_plan* plan, const float* noisy, float* x_out, int B, int H, int W,
                      const int32_t* t_list, int n_iters,
                      const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                      uint64_t seed, int64_t sample_offset, int flags,
                      void* workspace, size_t workspace_bytes, void* stream);

/* CONTINUOUS BATCHING: the sampler loop with per-slot timesteps.  The B samples of the call are independent SLOTS: each has its
 * own condition image, its own timestep in every row and its own noise counter words.  Row i runs ONE forward over all B slots
 * with t_rows[i][b] as slot b's timestep, then the update of mi_denoise / mi_denoise_seeded per slot (same operation order, same
 * rounding: a table whose columns all equal a t_list gives, with x preset to the condition, mi_denoise's bits at the same B).
 *   cond          device fp32 [B,C,H,W]: the slots' condition images, read by every row
 *   x             device fp32 [B,C,H,W], IN/OUT and NOT initialised by the call: a caller starting a slot copies its condition
 *                 image into it; a slot continues across calls.  Must not overlap cond
 *   t_rows        HOST int32 [n_rows][B]; -1 = idle: x[b] keeps its bits, nothing is drawn or written for it (the network still
 *                 runs over the slot at time row 0, so its cond and x must hold finite values).  Within a call a slot is active
 *                 on a prefix of the rows: a new image joins at a call boundary
 *   iter_base     HOST int32 [B] or NULL (all 0): rows of slot b already run in earlier calls
 *   sample_index  HOST int64 [B] or NULL (0 .. B-1): the global image index of slot b
 *   step_noise    device fp32 [n_rows,B,C,H,W] (0.5-scaled, as mi_denoise's) or NULL; entries of idle rows and of t == 0 are ignored
 *   seeded != 0   the noise term of every active t > 0 update is drawn as mi_denoise_seeded draws it, with counter words
 *                 c1 = low 32 bits of sample_index[b], c2 = iter_base[b] + i, c3 = 0, c0 and the key as specified above
 *   flags         MI_CLAMP_EPS, MI_NO_SPLIT as in mi_denoise.  The batch splits exactly as there: same sub-batches, same phase
 *                 offset, joined before the call returns; sub-batch h takes columns [h*B/parts, (h+1)*B/parts) of every table
 * The per-row coefficients are computed on the host in fp32 in the reference's order and reach the device, with the counter
 * words and the active flag, as kernel arguments of a small launch per row (<= 32 slots each) that writes them into the
 * workspace: the host tables are not read after the call returns, and the loop has no host synchronisation.
 * workspace: mi_workspace_bytes(B, H, W).  The status word is cleared once per call.  n_rows == 0: MI_OK, nothing is enqueued.
 * MI_EINVAL before any GPU work (mi_last_error names the limit): a null argument; n_rows < 0; a timestep outside
 * [-1, noise_steps); a slot active again after an idle row; iter_base[b] < 0 or iter_base[b] + n_rows > 2^31 - 1;
 * sample_index[b] < 0; seeded with C*H*W >= 2^32; seeded together with step_noise; x overlapping (or equal to) cond. */
int mi_denoise_slots(mi_plan* plan, const float* cond, float* x, int B, int H, int W,
                     const int32_t* t_rows, int n_rows, const int32_t* iter_base, const int64_t* sample_index,
                     const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                     const float* step_noise, int seeded, uint64_t seed, int flags,
                     void* workspace, size_t workspace_bytes, void* stream);

/* The same loop with every slot a VIRTUAL SAMPLE: slot b carries its own member word and the frame of its element index, the two
 * things a member of mi_denoise_ensemble and a tile of mi_denoise_tiled differ in from a whole image.  mi_denoise_slots is this
 * call with member == frame == NULL: same bits, same launches; every rule above holds, in its order.
 *   member        HOST int64 [B] or NULL (all 0): counter word c3 of slot b, 0 <= member[b] < 2^32
 *   frame         HOST uint32 [B][3] or NULL: (pitch, plane, origin) of slot b; NULL = (W, H*W, 0).  The element index (counter
 *                 word c0) of channel c, row y, column x of the slot is  c * plane + y * pitch + x + origin  in uint32 arithmetic
 * With frame[b] = (Wi, Hi*Wi, y0*Wi + x0) slot b draws what mi_denoise_tiled draws for the tile at origin (y0, x0) of an Hi x Wi
 * image whose global index is sample_index[b]: the noise field belongs to the image, not to the tiling, so the tiles of one image
 * may sit in any slots, join at any call and run at different rows.  With member[b] = m it draws what mi_denoise_ensemble draws
 * for member m (member_offset included) of image sample_index[b].  With a batch-invariant plan a slot's result is therefore the
 * tile's or the member's bits in those calls, whatever shares the batch.
 * Both tables are read before the call returns, as the others are (they travel in the per-row records, 48 bytes a slot).
 * Further MI_EINVAL cases, before any GPU work and after the rules of mi_denoise_slots up to "seeded together with step_noise":
 * member or frame given without seeded (they are the generator's counter words; a step_noise tensor is already per slot);
 * member[b] outside [0, 2^32); a frame row with pitch < W; with origin + (H-1)*pitch + W > plane (in 64 bits: the slot would
 * leave its channel plane); with C*plane >= 2^32. */
int mi_denoise_slots_virtual(mi_plan* plan, const float* cond, float* x, int B, int H, int W,
                             const int32_t* t_rows, int n_rows, const int32_t* iter_base, const int64_t* sample_index,
                             const int64_t* member, const uint32_t* frame,
                             const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                             const float* step_noise, int seeded, uint64_t seed, int flags,
                             void* workspace, size_t workspace_bytes, void* stream);

/* The values mi_denoise_seeded draws, as a tensor (no plan needed): dst device fp32 [n_iters,B,C,H,W] <- 0.5 * z of
 * (seed, sample_offset + b, i, element), i.e. already 0.5-scaled as mi_denoise's `step_noise` expects.  Replay and export:
 * mi_denoise with this tensor equals mi_denoise_seeded bit for bit.  Every iteration is filled (the t == 0 entry is ignored
 * by mi_denoise).  MI_EINVAL: sample_offset < 0, C*H*W >= 2^32, B or n_iters > 65535.  Asynchronous on `stream`. */
int mi_step_noise_fill(float* dst, int n_iters, int B, int C, int H, int W,
                       uint64_t seed, int64_t sample_offset, void* stream);
/* The same for ensemble member `member` (0 <= member < 2^32, else MI_EINVAL) of every image: counter word c3 = member.
 * member == 0 is mi_step_noise_fill.  mi_denoise with this tensor replays member `member` of mi_denoise_ensemble. */
int mi_step_noise_fill_member(float* dst, int n_iters, int B, int C, int H, int W,
                              uint64_t seed, int64_t sample_offset, int64_t member, void* stream);

/* ENSEMBLES of the stochastic (cddpm) sampler: `members` seeded draws per image in one call, their per-pixel mean and
 * unbiased standard deviation (the reference returns one draw, cddpmModels.py:281-308; a caller who wants several loops).
 * A "virtual sample" is one (image b, member m) pair; the virtual batch is image-major, v = b * members + m, so the member
 * outputs [B,members,C,H,W] ARE the virtual batch.  Virtual sample v draws the step noise of the specification above with
 *   global image index  sample_offset + v / members        (counter word c1)
 *   member index        member_offset + v % members        (counter word c3)
 * so member 0 of image b is what mi_denoise_seeded computes for that image, and -- with a batch-invariant plan -- every member
 * output is a function of (seed, image, member) alone: not of B, members, pass_samples or the stream.
 * The B * members virtual samples run through mi_denoise's sampler loop in passes of at most pass_samples consecutive virtual
 * samples (the last pass may be shorter); each pass is split over two streams as a mi_denoise batch of that size is.  One
 * reduce launch (mi_ensemble_reduce) follows the last pass.
 *   noisy        device fp32 [B,C,H,W]; never written
 *   mean_out     device fp32 [B,C,H,W] or NULL
 *   std_out      device fp32 [B,C,H,W] or NULL; needs members >= 2
 *   samples_out  device fp32 [B,members,C,H,W] or NULL: the member outputs (NULL: they live in the workspace)
 *   seed, sample_offset   as mi_denoise_seeded (sample_offset counts IMAGES)
 *   member_offset  member index of member 0 of this call.  members == 1, member_offset = m, samples_out = x, mean_out =
 *                std_out = NULL is "run member m only": the single-member form
 *   pass_samples  virtual samples per pass (>= 1); the workspace grows with it (mi_ensemble_workspace_bytes)
 *   flags        as mi_denoise (MI_NO_SPLIT: every pass as one program)
 * MI_EINVAL before any GPU work, with the limit named in mi_last_error: members < 1; member_offset < 0; member_offset +
 * members > 2^32 (4294967296: the member index is one 32-bit counter word); pass_samples < 1; no output pointer; std_out with
 * members < 2; any two of noisy, mean_out, std_out, samples_out overlapping; sample_offset < 0; C*H*W >= 2^32; B > 65535 or B * members > 2^31 - 1 (2147483647:
 * grid of the reduce kernel, 32-bit virtual index).
 * The status word (mi_status) is cleared once per call and accumulates over the passes.  Allocates nothing; asynchronous. */
int mi_denoise_ensemble(mi_plan* plan, const float* noisy, float* mean_out, float* std_out, float* samples_out,
                        int B, int members, int H, int W,
                        const int32_t* t_list, int n_iters,
                        const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                        uint64_t seed, int64_t sample_offset, int64_t member_offset, int pass_samples, int flags,
                        void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of workspace mi_denoise_ensemble needs: the sampler workspace of a pass (>= mi_workspace_bytes of pass_samples
 * virtual samples) + the pass's condition images + -- unless samples_external != 0, i.e. samples_out is given -- the member
 * outputs, B * members * C*H*W * 4 bytes.  Host only, and answered from the planner alone: it works before mi_unet_finalize
 * too.  0 on bad arguments (mi_last_error says which). */
size_t mi_ensemble_workspace_bytes(mi_plan* plan, int B, int members, int H, int W, int pass_samples, int samples_external);

/* The reduction of mi_denoise_ensemble on its own (no plan needed; a caller who gathered members from several GPUs reduces
 * them with the same arithmetic): samples device fp32 [B,members,chw] -> mean_out [B,chw] and, if not NULL, std_out [B,chw]
 * (members >= 2).  THE ARITHMETIC (fixed, per pixel, independent of the launch geometry): in double precision, every operation
 * rounded to nearest on its own, no fused multiply-add,
 *   s = 0; for m = 0 .. members-1: s += (double)x[m];      mean64 = s / members
 *   q = 0; for m = 0 .. members-1: d = (double)x[m] - mean64; q += d * d
 *   mean = (float)mean64        std = (float)sqrt(q / (members - 1))       (unbiased)
 * MI_EINVAL: B outside [1, 65535], members < 1, chw outside [1, 2^32), null samples / mean_out, std_out with members < 2.
 * samples, mean_out and std_out must not overlap (the kernel reads the samples while it writes the other two). */
int mi_ensemble_reduce(const float* samples, int B, int members, int64_t chw, float* mean_out, float* std_out, void* stream);

/* QUANTILE MAPS over the members of an ensemble (no plan needed): samples device fp32 [B,members,chw] -> out [B,nq,chw], per pixel
 * the nq quantiles q[0 .. nq-1] (host doubles in [0, 1]) of its members.  Every member of this network is clamped to [0, 1], so
 * the per-pixel distribution is skewed and piles up at the clamp: a median and an interval (0.05 .. 0.95) describe it where
 * mean +- std does not.  THE ARITHMETIC (fixed, per pixel, independent of the launch geometry, the vector width and the alignment
 * path), over the member values x_0 .. x_{K-1}, K = members:
 *   NaN          if any x_m is NaN, every quantile of the pixel is the canonical quiet NaN 0x7FC00000 (numpy's rule: nothing is
 *                silently dropped)
 *   sort         else ascending in the total order of the unsigned key  k = bits ^ (sign ? 0xFFFFFFFF : 0x80000000):
 *                -inf < ... < -0.0 < +0.0 < ... < +inf; ties carry identical bits, so the sorted s_0 .. s_{K-1} is unique
 *   interpolate  per level q, in double precision, every operation rounded to nearest on its own, no fused multiply-add:
 *                  pos = q * (double)(K-1);  lo = (int)floor(pos);  hi = min(lo+1, K-1);  g = pos - (double)lo
 *                  out = (float)( (double)s_lo + g * ((double)s_hi - (double)s_lo) )
 *                K == 1: every quantile is x_0, bit for bit.  A NaN the formula itself makes of infinite members (inf - inf,
 *                0 * inf) is stored as 0x7FC00000 too.
 * So, for finite members, q = 0 is the minimum and q = 1 the maximum, a q whose pos is an integer returns a member's value (equal in
 * value, not always in bits: g = 0 turns a -0.0 into +0.0 when K > 1), and the levels of a pixel are non-decreasing in q.  An
 * infinite member at or next to the position makes 0 * inf or inf - inf, i.e. NaN: q = 0 over a pixel with a -inf member is NaN.
 * None of this arises for outputs clamped to [0, 1].  This is numpy.quantile(x.astype(float64), q) ("linear") up to its different rounding of the
 * interpolation: within 1 fp32 ulp of it for members in [0, 1) (tests/test_quantiles_cpu.py).
 * The kernel sorts a pixel's members in registers: members <= 64 (mean and std have no such limit).  The levels travel as kernel
 * arguments: 1 <= nq <= 8; the call allocates nothing and is asynchronous.
 * MI_EINVAL before any GPU work, the rule named in mi_last_error: B outside [1, 65535], members < 1, chw outside [1, 2^32),
 * members > 64, nq outside [1, 8], null q / samples / out, a q[i] that is NaN or outside [0, 1].
 * samples and out must not overlap. */
int mi_ensemble_quantiles(const float* samples, int B, int members, int64_t chw,
                          const double* q, int nq, float* out, void* stream);

/* ENSEMBLE SCORES against a truth image (no plan needed): do the uncertainty maps of an ensemble mean anything?  samples device fp32
 * [B,members,chw] and truth device fp32 [B,chw] -> per image the sums behind the CRPS, the error of the mean and the spread, the rank
 * histogram of the truth among the members and, per quantile level, how often the truth lies below that quantile map -- one pass over
 * the members, nothing copied to the host but these few numbers.
 * THE ENSEMBLE SCORES (fixed; independent of the launch geometry, the vector width and the alignment path).  K = members,
 * 1 <= K <= 64; levels q[0 .. nq-1], host doubles in [0, 1], 0 <= nq <= 8.  A pixel e of image b has x_m = samples[b][m][e] and
 * y = truth[b][e].
 *   invalid      a pixel whose y or any x_m is not finite (NaN, +-inf) is INVALID: it adds 1 to invalid[b] and nothing else, and its
 *                crps_map value is the canonical quiet NaN 0x7FC00000.
 *   valid        every other pixel; double precision, every operation rounded to nearest on its own, no fused multiply-add:
 *     mean, var  exactly mi_ensemble_reduce's arithmetic, members in index order:
 *                  s = 0; s += (double)x_m;  mean64 = s / K;   v = 0; d = (double)x_m - mean64; v += d * d;
 *                  var = v / (K - 1), or 0 for K == 1;         dm = mean64 - (double)y;  se = dm * dm
 *     sort       ascending by the order key of mi_ensemble_quantiles: s_0 .. s_{K-1}
 *     CRPS       a = 0; for i = 0 .. K-1: a += |(double)s_i - (double)y|
 *                g = 0; for i = 0 .. K-1: g += (double)(2i - K + 1) * (double)s_i     (the product is exact: 7 bits x 24 bits)
 *                sum_i sum_j |s_i - s_j| = 2 g, so the CRPS of the members' empirical distribution, mean|X - y| - mean|X - X'| / 2, is
 *                  c = a / (double)K - g / (double)(K*K)            crps_map = (float)c
 *     rank       float comparisons (so -0.0 == +0.0):  lt = #{m : x_m < y},  eq = #{m : x_m == y};  rank_hist[b][2*lt + eq] += 1.
 *                That is the mid-rank lt + eq/2 in half steps, bins 0 .. 2K: an exact integer rule with no random tie-break (ties are
 *                the common case here: every member is clamped to [0, 1]).  A calibrated ensemble without ties fills the even bins
 *                0, 2, .., 2K evenly; an under-dispersed one piles up in bins 0 and 2K.
 *     coverage   per level i, Q_i = the quantile of mi_ensemble_quantiles, bit for bit (fp32):
 *                  counts[b][i][0] += (y < Q_i)        counts[b][i][1] += (y <= Q_i)          (float comparisons)
 *                so the share of valid pixels inside [Q_lo, Q_hi] is (counts[hi][1] - counts[lo][0]) / valid.
 *   sums         per image A = sum a, G = sum g, E = sum se, V = sum var over its valid pixels, in double, no atomics, in ONE order:
 *                - the chw elements of an image are cut into chunks of 1024 consecutive elements (the last one may be partial);
 *                - in a chunk, lane j = 0 .. 255 owns elements 4j .. 4j+3 and adds them in that order starting from 0; invalid and
 *                  absent pixels add nothing;
 *                - the 256 lane sums are folded by the tree  for off = 128, 64, .., 1: v[j] += v[j + off]  for j < off;
 *                - an image's chunk sums are added one by one, starting from 0, in chunk order.
 *                The caller composes, with N = chw - invalid[b]:  crps = A/(K N) - G/(K^2 N);  the fair (unbiased in K) form
 *                crps_fair = A/(K N) - G/(K (K-1) N);  rmse = sqrt(E/N);  spread = sqrt(V/N)  (rmse ~ spread: calibrated).
 *   integers     invalid, rank_hist and counts are exact integers: their order is free (64-bit integer atomics).
 * Arguments
 *   sums         device double [B][4] = (A, G, E, V), 8-byte aligned
 *   invalid      device uint64 [B];  rank_hist  device uint64 [B][2*members+1];  both 8-byte aligned.  The call zeroes its integer
 *                outputs itself, on the stream
 *   counts       device uint64 [B][nq][2], 8-byte aligned; NULL if and only if nq == 0
 *   crps_map     device fp32 [B][chw] or NULL (skipped)
 *   workspace    mi_ensemble_scores_workspace_bytes (the chunk sums, double [B][chunks][4]), 8-byte aligned; the query answers 0 on
 *                sizes the call refuses
 * Every member is read once, as 16-byte words when chw is a multiple of 4 and samples, truth and crps_map are 16-byte aligned, element
 * by element otherwise: the same bits either way.  Allocates nothing; asynchronous; needs no plan.
 * MI_EINVAL before any GPU work, the rule named in mi_last_error, judged in this order: B outside [1, 65535]; members outside
 * [1, 64]; chw outside [1, 2^32); nq outside [0, 8]; a level that is NaN or outside [0, 1]; a null samples, truth, sums, invalid,
 * rank_hist or workspace (or q with nq > 0); counts and nq disagreeing; sums, invalid, rank_hist, counts or workspace not 8-byte
 * aligned, samples, truth or crps_map not 4-byte aligned; workspace_bytes below the query's answer; any output (workspace included)
 * overlapping an input or another output. */
size_t mi_ensemble_scores_workspace_bytes(int B, int members, int64_t chw);
int mi_ensemble_scores(const float* samples, const float* truth, int B, int members, int64_t chw,
                       const double* q, int nq,
                       double* sums, uint64_t* invalid, uint64_t* rank_hist, uint64_t* counts, float* crps_map,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ENSEMBLE MODES (no plan needed): what varies TOGETHER?  The std and quantile maps say how much a pixel varies, the scores whether
 * that amount is calibrated; neither tells a global brightness shift from an edge that moves or a structure that comes and goes.
 * The principal components of the members do: the leading eigenvectors of their covariance, each shown as an image in grey-level
 * units.  With K <= 64 members the covariance never exists: the K x K Gram matrix of the centred members is a reduction over the
 * pixels (mi_ensemble_gram), its eigenvectors are a host matter (C callers bring their own symmetric eigensolver), and the modes
 * are one projection of the centred members onto the scaled eigenvectors (mi_ensemble_project).  Channels are pooled: an element
 * is one of the chw values of an image.
 * THE ENSEMBLE MODES (fixed; independent of the launch geometry, the vector width and the alignment path).  K = members,
 * 2 <= K <= 64.  An element e of image b has x_m = samples[b][m][e].  Double precision, every operation rounded to nearest on its
 * own, no fused multiply-add.
 *   invalid      an element with a member that is not finite (NaN, +-inf) is INVALID: it adds 1 to invalid[b] and nothing to the Gram
 *                matrix, and its projected value is the canonical quiet NaN 0x7FC00000 in every mode.
 *   centring     every other element, exactly mi_ensemble_reduce's mean, members in index order:
 *                  s = 0; s += (double)x_m;  mean64 = s / K;      d_m = (double)x_m - mean64
 *   Gram         G[i][j] = sum over the valid elements of d_i * d_j for i <= j: the product is rounded, then added.  G[j][i] = G[i][j].
 *   sums         per image and entry (i, j), no atomics, in ONE order:
 *                - the chw elements of an image are cut into chunks of 4096 consecutive elements (the last one may be partial);
 *                - a chunk is 16 rounds of 256 elements; lane l = 0 .. 63 owns elements 256 r + 4 l .. 256 r + 4 l + 3 of round
 *                  r = 0 .. 15 and adds its 64 products in increasing element order starting from 0; invalid and absent elements
 *                  add nothing;
 *                - the 64 lane sums are folded by the tree  for off = 32, 16, .., 1: v[l] += v[l + off]  for l < off;
 *                - an image's chunk sums are added one by one, starting from 0, in chunk order.
 *                (A chunk four times that of the scores: the tree runs over up to 2080 accumulators per chunk and is paid for by 64
 *                elements a lane.)
 *   projection   weights w[b][j][k], device doubles, j < M = n_modes, 1 <= M <= 8:
 *                  a = 0; for k = 0 .. K-1: a += w[b][j][k] * d_k;      out[b][j][e] = (float)a
 *                the product rounded, then added.  The weights are the caller's and should be finite.
 * With mu_j, v_j the eigenpairs of G (v_j of unit length) and w[j][k] = v_j[k] / sqrt(K - 1), out[b][j] is mode j in image units:
 * mean +- out[b][j] is a one-standard-deviation excursion along the j-th pattern, its variance is mu_j / (K - 1), and over all K - 1
 * modes sum_j out[b][j]^2 is the unbiased per-pixel variance.  Eigenvectors of (nearly) equal eigenvalues are not unique: any
 * rotation within their span is as good, so only the span of such modes is reproducible between solvers.
 * Arguments
 *   gram         device double [B][K][K], 8-byte aligned, written symmetric
 *   invalid      device uint64 [B], 8-byte aligned; the call zeroes it itself, on the stream
 *   workspace    mi_ensemble_gram_workspace_bytes, 8-byte aligned: the chunk sums of the upper triangle, double
 *                [B][chunks][K (K + 1) / 2], and for K > 8 the double mean of every element, double [B][chw] (K <= 8: one launch
 *                holds all members and computes the mean itself; above, the members are tiled in blocks of 8 and a pre-pass
 *                stores the mean once).  The query answers 0 on sizes the call refuses
 *   out          device fp32 [B][M][chw]
 * The members are read as 16-byte words when chw is a multiple of 4 and samples (and out) are 16-byte aligned, element by element
 * otherwise: the same bits either way.  Both calls allocate nothing, are asynchronous and need no plan.
 * MI_EINVAL before any GPU work, the rule named in mi_last_error, judged in this order.  mi_ensemble_gram: B outside [1, 65535];
 * members outside [2, 64]; chw outside [1, 2^32); a null samples, gram, invalid or workspace; gram, invalid or workspace not 8-byte
 * aligned, samples not 4-byte aligned; workspace_bytes below the query's answer; gram, invalid or the workspace overlapping samples
 * or each other.  mi_ensemble_project: B, members and chw as above; n_modes outside [1, 8]; a null samples, weights or out; weights
 * not 8-byte aligned, samples or out not 4-byte aligned; any two of samples, weights and out overlapping. */
size_t mi_ensemble_gram_workspace_bytes(int B, int members, int64_t chw);
int mi_ensemble_gram(const float* samples, int B, int members, int64_t chw, double* gram, uint64_t* invalid,
                     void* workspace, size_t workspace_bytes, void* stream);
int mi_ensemble_project(const float* samples, int B, int members, int64_t chw, const double* weights, int n_modes,
                        float* out, void* stream);

/* CHANNEL RESPONSES (no plan needed): is a faint signal easier or harder to see after the run?  The task-based answer is a model
 * observer: many noisy realisations with and without a known signal go through the system, and a channelized Hotelling observer is
 * asked how well it separates the two classes.  Its statistics are a host matter on [rows][C] doubles; its hot path is this call: the
 * responses of N planes at L locations to C channel templates, i.e. N * L * C dot products over R x R regions of interest (ROIs), in
 * one fixed order.
 * THE CHANNEL RESPONSES (fixed; independent of the launch geometry, the load width and the alignment).  The ROI of the centre
 * (cy, cx) = centres[l] has its origin at y0 = cy - R / 2, x0 = cx - R / 2 (integer division) and covers rows y0 .. y0 + R - 1 and
 * columns x0 .. x0 + R - 1: the centre pixel has ROI index (R / 2, R / 2), R odd or even.  With p = y R + x, u_c[p] =
 * channels[c][y][x] and g_p = (double)x[n][y0 + y][x0 + x]; double precision, every operation rounded to nearest on its own, no
 * fused multiply-add:
 *   lanes        lane j = 0 .. 63 starts from 0 and adds u_c[p] * g_p (the product rounded, then added) for p = j, j + 64, j + 128, ..
 *                below R * R, in increasing order;
 *   tree         the 64 lane sums are folded by  for off = 32, 16, .., 1: v[j] += v[j + off]  for j < off;
 *   response     out[n][l][c] is the root v[0].
 *   invalid      an ROI that holds a pixel that is not finite (NaN, +-inf) is INVALID: invalid[n][l] = 1 and its C responses are the
 *                canonical quiet NaN 0x7FF8000000000000.  Every other ROI has invalid[n][l] = 0.  A pixel outside every ROI is never
 *                read and has no effect.  The channels are the caller's and should be finite.
 * ROIs may overlap or repeat; each is computed on its own.
 * Arguments
 *   x            device fp32 [N][H][W], contiguous planes, 4-byte aligned
 *   centres      HOST int32 [L][2] as (cy, cx), as the timestep lists of the sampler calls are host arrays: read and judged before
 *                any GPU work and not needed after the call returns.  The origins travel as kernel arguments, 512 locations a
 *                launch, so the call needs no workspace
 *   channels     device double [C][R][R], 8-byte aligned
 *   out          device double [N][L][C], 8-byte aligned
 *   invalid      device uint32 [N][L], 4-byte aligned; every entry is written
 * The planes are read element by element whatever the alignment: there is one load path.  The call allocates nothing, is
 * asynchronous and needs no plan.
 * MI_EINVAL before any GPU work, the rule named in mi_last_error, judged in this order: N outside [1, 65535]; H outside [1, 32768];
 * W outside [1, 32768]; R outside [4, 128]; L outside [1, 4096]; C outside [1, 32]; an ROI that leaves the image -- y0 < 0, x0 < 0,
 * y0 + R > H or x0 + R > W: refused, not clipped, the first such centre named (a null centres is "null argument" here: the rule
 * reads it); a null x, channels, out or invalid; channels or out not 8-byte aligned; x or invalid not 4-byte aligned; any two of x,
 * channels, out and invalid overlapping. */
int mi_channel_responses(const float* x, int N, int H, int W, const int32_t* centres, int L, int R, const double* channels, int C,
                         double* out, uint32_t* invalid, void* stream);

/* NOISE POWER SPECTRUM (no plan needed): what does the remaining noise look like?  The per-pixel scores above say how large a
 * residual or an ensemble's spread is; the noise power spectrum (NPS) says at which spatial frequencies it lives.  Welch's method as
 * in IEC 62220-1: overlapping regions of interest (ROIs) are detrended, windowed, transformed, their periodograms averaged and the
 * average binned by radial frequency.  a device fp32 [B,K,C,H,W], b device fp32 [B,C,H,W] or NULL (broadcast over K).
 * THE NOISE POWER SPECTRUM (fixed; independent of the launch geometry, the vector width and the alignment path).
 *   field        f = a - b, ONE fp32 subtraction (b == NULL: f = a).  A group g = b*C + c is a (b, c) pair; its realisations are
 *                the K members.
 *   ROIs         size R = roi in {32, 64, 128}, step S >= 1; origins (iy*S, ix*S), iy < ny = (H-R)/S + 1, ix < nx = (W-R)/S + 1
 *                (integer divisions); no partial ROIs.  The ROIs of a group are numbered n = (m*ny + iy)*nx + ix, m the member.
 *   skipped      an ROI holding a NaN or an Inf in f is SKIPPED: it adds 1 to rois_skipped[g] and nothing else.  Every other ROI is
 *                USED (rois_used[g]).  Only f is judged; a non-finite value is never folded into a sum.
 *   detrend      0 none: d = f.  1 mean, 2 plane: in double, every operation rounded to nearest on its own, no fused multiply-add,
 *                with xc = x - (R-1)/2, yc = y - (R-1)/2 (exact):
 *                  row sums     s0[y] = 0; s0[y] += (double)f[y][x]        s1[y] = 0; s1[y] += xc * (double)f[y][x]     x = 0 .. R-1
 *                  ROI sums     t0 = 0; t0 += s0[y]     tx = 0; tx += s1[y]     ty = 0; ty += yc * s0[y]                y = 0 .. R-1
 *                  m = t0 / R^2;   ax = tx / D,  ay = ty / D  with  D = R * (R (R^2 - 1) / 12)  (plane)  or  ax = ay = 0  (mean)
 *                  d = (float)((double)f - ((m + ax*xc) + ay*yc)), rounded to fp32 once
 *   window       an optional separable table w[R] (host floats): d = (d * w[y]) * w[x], each fp32 product rounded on its own.
 *                S_w = (sum_i (double)w[i]^2)^2, the sum in index order from 0; without a window S_w = R^2.
 *   transform    the 2-D DFT of size R x R in fp32 by radix-2 decimation in time.  Twiddles T[t] = ((float)cos(2 pi t / R),
 *                (float)(-sin(2 pi t / R))), t < R/2, computed on the host in double with the angle 2.0 * pi * t / R evaluated left
 *                to right, and rounded to fp32; no device sincos.  The ROI is stored at [bitrev(y)][bitrev(x)] (bit reversal over
 *                log2 R bits) with imaginary part 0.  A pass over a line z[0 .. R-1] is, for s = 1 .. log2 R, half = 2^(s-1), for
 *                every k a multiple of 2^s and j < half, with (wr, wi) = T[j * R / 2^s], A = z[k+j], X = z[k+j+half]:
 *                  tr = wr*X.re - wi*X.im;   ti = wr*X.im + wi*X.re        (4 multiplications, 2 additions, no contraction)
 *                  z[k+j] = (A.re + tr, A.im + ti);   z[k+j+half] = (A.re - tr, A.im - ti)
 *                (also for the unit twiddle T[0]).  First every row is passed in full, then the columns u = 0 .. R/2: the rows are
 *                transforms of real data, so the other columns are taken as the mirror, P[v][u] = P[(R-v) % R][R-u] for u > R/2.
 *   periodogram  P[v][u] = (double)re * (double)re + (double)im * (double)im  (the products are exact, the sum is rounded once).
 *   accumulation per group and entry (v, u), in double, no atomics, in ONE order: the ROIs n = 0, 1, .. are cut into chunks of 16
 *                consecutive ROIs (skipped ones included; they add nothing; the last chunk may be partial); a chunk's used ROIs are
 *                added in order of n starting from 0; the group's chunk sums are added one by one, starting from 0, in chunk order.
 *   result       nps[g][v][u] = (scale * sum) / ((double)rois_used[g] * S_w), DFT order (index 0 is DC), double [B,C,R,R].  White
 *                noise of variance s^2 has a flat NPS of scale * s^2 (unit pixel pitch; frequencies in cycles per pixel), and
 *                sum(nps) / R^2 is scale times the mean windowed variance (Parseval).  A group with no used ROI is the quiet NaN
 *                0x7FF8000000000000 in every nps and radial entry.
 *   radial       fu = u < R/2 ? u : u - R, fv likewise, d2 = fu^2 + fv^2.  Entry (v, u) belongs to the integer bin r with
 *                (2r-1)^2 <= 4*d2 < (2r+1)^2 (for r = 0 only the upper bound counts): r = floor(sqrt(d2) + 1/2) in integers.
 *                Bins r = 0 .. R/2; the corners beyond are dropped.  radial[g][r] = the double sum of the bin's nps entries in
 *                row-major (v, then u) order starting from 0, divided by their number radial_count[r]; an empty bin is the quiet NaN
 *                above.  Flag MI_NPS_EXCLUDE_AXES leaves out every entry with fu == 0 or fv == 0 (detector fixed-pattern lines
 *                live on the axes); bin 0 is then empty.
 * Arguments
 *   window       HOST fp32 [roi] or NULL; it and the twiddles travel as kernel arguments
 *   nps          device double [B*C][roi][roi];  radial  device double [B*C][roi/2+1];  radial_count  device int64 [roi/2+1];
 *   rois_used, rois_skipped  device int64 [B*C];  all 8-byte aligned
 *   workspace    mi_noise_power_spectrum_workspace_bytes: the chunk sums of the half plane, double [B*C][chunks][roi*(roi/2+1)], and
 *                the chunks' used counts, int64 [B*C][chunks]; 8-byte aligned; the query answers 0 on sizes the call refuses
 * An ROI is read as 16-byte words when W is a multiple of 4 and its first element is 16-byte aligned (judged for a and for b on their
 * own) and element by element otherwise: the same bits.
 * Three launches on `stream` (the ROIs; the chunk sums, scaling and mirror; the radial bins); allocates nothing; asynchronous.
 * MI_EINVAL before anything is read, the rule named in mi_last_error, judged in this order: roi outside {32, 64, 128}; step < 1; B,
 * K or C < 1; B*C > 65535; H < roi or W < roi; ROIs per member or chunks >= 2^31; detrend outside {0, 1, 2}; unknown flags; scale
 * not finite; a null a, nps, radial, radial_count, rois_used, rois_skipped or workspace; an output or the workspace not 8-byte
 * aligned, a or b not 4-byte aligned; workspace_bytes below the query's answer; any output (workspace included) overlapping an input
 * or another output; a window entry that is not finite. */
#define MI_NPS_DETREND_NONE  0
#define MI_NPS_DETREND_MEAN  1
#define MI_NPS_DETREND_PLANE 2
#define MI_NPS_EXCLUDE_AXES  1
size_t mi_noise_power_spectrum_workspace_bytes(int B, int K, int C, int H, int W, int roi, int step);
int mi_noise_power_spectrum(const float* a, const float* b, int B, int K, int C, int H, int W, int roi, int step, int detrend,
                            const float* window, double scale, int flags,
                            double* nps, double* radial, int64_t* radial_count, int64_t* rois_used, int64_t* rois_skipped,
                            void* workspace, size_t workspace_bytes, void* stream);

/* CROSS SPECTRUM (no plan needed): at which spatial frequencies does the signal survive?  The NPS above is the spectrum of ONE
 * field; resolution needs two: the Welch cross-spectrum S_xy of a truth x and an output y (or of two independent draws of an
 * ensemble) beside their auto-spectra S_xx, S_yy.  From the radial averages follow, on the host, the signal transfer
 * Re S_xy / S_xx (how much of x's amplitude at a frequency is in y: the MTF-like curve of a nonlinear, content-adaptive denoiser,
 * for which an edge-phantom MTF is not defined) and the Fourier ring correlation Re S_xy / sqrt(S_xx S_yy).
 * x device fp32 [B,Kx,C,H,W], y device fp32 [B,Ky,C,H,W] with Kx, Ky in {K, 1}, K = max(Kx, Ky).
 * THE CROSS SPECTRUM (fixed; independent of the launch geometry, the vector width and the alignment path).  Everything not named
 * here -- ROIs and their numbering, detrend, window and S_w, twiddles, storage order, the butterfly, chunks, radial bins -- is THE
 * NOISE POWER SPECTRUM's, applied to x and to y each on its own.
 *   fields       x and y as given: there is no subtraction.  A field with one realisation (Kx or Ky == 1 < K) is broadcast over the
 *                K members.  A group g = b*C + c is a (b, c) pair; ROI n = (m*ny + iy)*nx + ix pairs member m of x (or its only one)
 *                with member m of y at the same position.
 *   skipped      an ROI is SKIPPED when x OR y holds a NaN or an Inf inside it; it is counted once in rois_skipped[g].
 *   detrend, window   the NPS's operations on the ROI of x -> dx and, with its own sums and coefficients, on that of y -> dy.
 *   transform    ONE complex transform per ROI of z = (dx, dy): dx is the real part, dy the imaginary part, stored at
 *                [bitrev(y)][bitrev(x)].  The NPS pass over all R rows, then over ALL R columns (the row transforms of a complex
 *                field are not Hermitian: there is no half-column shortcut).  Z[v][u] is the result in DFT order.
 *   separation   per entry (v, u) of the half plane u <= R/2, in double: Z1 = Z[v][u], Z2 = Z[(R-v)%R][(R-u)%R], (x1, y1) and
 *                (x2, y2) their fp32 components converted to double.  Every product of two of them is exact; every sum is rounded
 *                on its own; no fused multiply-add; the factors 2, 1/2 and 1/4 are exact:
 *                  n1 = x1*x1 + y1*y1        n2 = x2*x2 + y2*y2
 *                  c  = x1*x2 - y1*y2        s  = x1*y2 + y1*x2                     (Z1 * Z2)
 *                  Sxx = ((n1 + n2) + 2c) / 4        Syy = ((n1 + n2) - 2c) / 4
 *                  Re Sxy = s / 2                    Im Sxy = (n1 - n2) / 4         (Sxy = X * conj Y)
 *                (from X = (Z1 + conj Z2) / 2 and Y = (Z1 - conj Z2) / (2i), the transforms of the two real fields).
 *   accumulation four double sums per group and entry, each in the NPS's ONE order (chunks of 16 ROIs; a chunk's used ROIs in order of
 *                n from 0; the chunk sums one by one from 0 in chunk order; no atomics).
 *   result       plane[q][g][v][u] = sum / ((double)rois_used[g] * S_w), q = 0 Sxx, 1 Syy, 2 Re Sxy, 3 Im Sxy, DFT order.  For
 *                0 < u < R/2 the entry ((R-v)%R, R-u) is the copy of (v, u) for Sxx, Syy and Re Sxy and its negation for Im Sxy
 *                (Sxy(-f) = conj Sxy(f)).  A group with no used ROI is the quiet NaN 0x7FF8000000000000 in every plane and radial
 *                entry.
 *   radial       the NPS's bins and order, MI_NPS_EXCLUDE_AXES included, over each of the four planes: radial[q][g][r].
 * Accuracy: the fp32 transform's rounding error is relative to the COMBINED energy of the two fields, sum (Sxx + Syy): against
 * float64 arithmetic on the same detrended, windowed ROIs, sum |S - S*| / sum (Sxx* + Syy*) <= 2 rho + rho^2 for each of the four
 * quantities (rho: Higham, Theorem 24.2, as for the NPS; 8.3e-6, 9.9e-6, 1.15e-5 for R = 32, 64, 128; measured: about 1e-7).  A
 * field much weaker than its partner therefore inherits the partner's rounding error, about 1e-7 of the STRONGER amplitude: scale
 * such a pair to comparable size first (the curves are ratios).
 * Arguments
 *   window       HOST fp32 [roi] or NULL, as for the NPS
 *   planes       device double [4][B*C][roi][roi];  radial  device double [4][B*C][roi/2+1];  radial_count  device int64 [roi/2+1];
 *   rois_used, rois_skipped  device int64 [B*C];  all 8-byte aligned
 *   workspace    mi_cross_spectrum_workspace_bytes: the chunk sums, double [B*C][chunks][4][roi*(roi/2+1)], and the chunks' used
 *                counts, int64 [B*C][chunks]; 8-byte aligned; the query answers 0 on sizes the call refuses
 * An ROI is read as 16-byte words when W is a multiple of 4 and its first element is 16-byte aligned (judged for x and for y on their
 * own) and element by element otherwise: the same bits.  x and y may overlap each other (y == x is the auto-spectrum twice).
 * Six launches on `stream` (the ROIs; the chunk sums, division and mirror; the radial bins of each plane); allocates nothing;
 * asynchronous.
 * MI_EINVAL before anything is read, the rule named in mi_last_error, judged in this order: Kx or Ky < 1; Kx != Ky with neither
 * equal to 1; then, with K = max(Kx, Ky), mi_noise_power_spectrum's rules from "roi outside {32, 64, 128}" to "unknown flags"; a null
 * x, y, planes, radial, radial_count, rois_used, rois_skipped or workspace; an output or the workspace not 8-byte aligned, x or y
 * not 4-byte aligned; workspace_bytes below the query's answer; any output (workspace included) overlapping an input or another
 * output; a window entry that is not finite. */
size_t mi_cross_spectrum_workspace_bytes(int B, int Kx, int Ky, int C, int H, int W, int roi, int step);
int mi_cross_spectrum(const float* x, const float* y, int B, int Kx, int Ky, int C, int H, int W, int roi, int step, int detrend,
                      const float* window, int flags,
                      double* planes, double* radial, int64_t* radial_count, int64_t* rois_used, int64_t* rois_skipped,
                      void* workspace, size_t workspace_bytes, void* stream);

/* TILED DENOISING: images of any size >= the tile, at their own resolution, as overlapping network-sized tiles (the reference
 * resizes every image to the training size first, Backend/run.py denoise_image_diffusion(..., img_size); nothing there tiles).
 * THE GEOMETRY (fixed), per axis with image length L, tile T, minimum overlap O, T <= L, 0 <= O <= T/2:
 *   n = 1 if L == T, else max(2, ceil((L - O) / (T - O)));   origin o_i = (i * (L - T)) / (n - 1) in integer division (o_0 = 0)
 *   window of position r in [0, T):  w(r) = min(r + 1, T - r, O + 1)  (integer);  a tile's weight at a pixel is wy * wx
 * Tiles of an image are numbered k = ky * nx + kx; virtual sample v = b * (ny * nx) + k is one (image, tile) pair.
 * mi_tile_geometry: host only, no plan: *n <- the tile count, origins[0 .. min(n, cap)) <- the origins (origins may be NULL).
 *   MI_EINVAL: T < 1, T > L, O < 0, O > T/2. */
int mi_tile_geometry(int L, int T, int O, int* n, int* origins, int cap);

/* dst device fp32 [n][C][th][tw] <- the tiles of virtual samples v0 .. v0 + n - 1 of noisy [B][C][H][W] (no plan needed; any
 * H, W, th, tw >= 1 with th <= H, tw <= W; n <= 65535 per call).  A copy: bit for bit the slices of the image. */
int mi_tile_extract(const float* noisy, int B, int C, int H, int W, int th, int tw, int oy, int ox, int v0, int n,
                    float* dst, void* stream);

/* out device fp32 [B][C][H][W] <- the blend of tiles [B][ny*nx][C][th][tw] (no plan needed).  THE ARITHMETIC (fixed, per pixel,
 * independent of the launch geometry, no atomics): over the tiles that cover the pixel, in ascending (ky, kx), in double
 * precision, every operation rounded to nearest on its own, no fused multiply-add,
 *   num += (double)(wy * wx) * (double)v;   den += (double)(wy * wx);   out = (float)(num / den)
 * A pixel under one tile gets that tile's value exactly.  tiles and out must not overlap.
 * MI_EINVAL: the geometry rules above, C*H*W >= 2^32, B * tiles > 2^31 - 1, overlap > 46339. */
int mi_tile_blend(const float* tiles, int B, int C, int H, int W, int th, int tw, int oy, int ox, float* out, void* stream);

/* Denoises B images [B,C,H,W] of any H >= th, W >= tw at their own size: every image is cut into ny * nx overlapping th x tw
 * tiles (th, tw: a shape the plan accepts), the B * ny * nx virtual samples run through mi_denoise's sampler loop in passes of
 * at most pass_samples consecutive virtual samples (extract, then the loop -- each pass split over two streams as a mi_denoise
 * batch of that size is, MI_NO_SPLIT honoured), and ONE blend launch follows the last pass.
 *   noisy      device fp32 [B,C,H,W]; never written
 *   image_out  device fp32 [B,C,H,W]
 *   tiles_out  device fp32 [B,ny*nx,C,th,tw] or NULL: the denoised tiles (NULL: they live in the workspace)
 *   t_list .. noise_steps   as mi_denoise
 *   seeded     0: no noise term (the DDIM variant);  != 0: the term is drawn as mi_denoise_seeded draws it, with the counter word
 *              c0 of a tile taken in the WHOLE image (specification above): the noise field belongs to the image, not to the
 *              tiling -- overlapping tiles see the same noise at the same pixel, a tile's noise is the crop of
 *              mi_step_noise_fill(.., B, C, H, W, seed, sample_offset), and th == H, tw == W is mi_denoise_seeded bit for bit
 *   seed, sample_offset   as mi_denoise_seeded (sample_offset counts IMAGES); c3 is 0
 *   pass_samples  virtual samples per pass (>= 1); the workspace grows with it (mi_tiled_workspace_bytes)
 *   flags      as mi_denoise
 * With a batch-invariant plan every tile output is a function of its crop (and, seeded, of seed, image and position) alone.
 * MI_EINVAL before any GPU work, with the limit named in mi_last_error: a tile that is no positive multiple of 2^(levels-1);
 * tile > image; overlap < 0 or > tile / 2; pass_samples < 1; any two of noisy, image_out, tiles_out overlapping;
 * sample_offset < 0; C*H*W >= 2^32; B * tiles > 2^31 - 1 (2147483647).
 * The status word (mi_status) is cleared once per call and accumulates over the passes.  Allocates nothing; asynchronous. */
int mi_denoise_tiled(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out,
                     int B, int H, int W, int th, int tw, int oy, int ox,
                     const int32_t* t_list, int n_iters,
                     const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                     int seeded, uint64_t seed, int64_t sample_offset, int pass_samples, int flags,
                     void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of workspace mi_denoise_tiled needs: the sampler workspace of a pass of tiles + the pass's condition tiles + -- unless
 * tiles_external != 0, i.e. tiles_out is given -- the tile outputs, B * ny*nx * C*th*tw * 4 bytes.  Host only, answered from the
 * planner alone: it works before mi_unet_finalize too.  0 on bad arguments (mi_last_error says which). */
size_t mi_tiled_workspace_bytes(mi_plan* plan, int B, int H, int W, int th, int tw, int oy, int ox, int pass_samples, int tiles_external);

/* ENSEMBLES OF TILED RUNS: `members` seeded draws of B full-resolution images, their per-pixel mean and unbiased standard
 * deviation at the images' own size.  Member m is mi_denoise_tiled's seeded run with the counter word c3 = member_offset + m
 * (c0: the pixel's index in the whole image, c1: sample_offset + image, as there), so member 0 at member_offset 0 IS that run,
 * bit for bit, and a tile of member m is mi_denoise of its crop with the crop of mi_step_noise_fill_member of member
 * member_offset + m.
 * Members are the OUTER loop: inside a member the B * ny * nx (image, tile) virtual samples run exactly as mi_denoise_tiled runs
 * them -- extract, then the sampler loop, in passes of at most pass_samples consecutive virtual samples, each pass split over two
 * streams as a mi_denoise batch of that size is (MI_NO_SPLIT honoured).  A pass never spans two members (the member word is a
 * launch constant of the update), so a member whose B * ny * nx is no multiple of pass_samples ends in a shorter pass.  ONE
 * mi_tile_blend_reduce launch follows the last pass of the last member.
 *   noisy        device fp32 [B,C,H,W]; never written
 *   mean_out     device fp32 [B,C,H,W] or NULL
 *   std_out      device fp32 [B,C,H,W] or NULL; needs members >= 2
 *   samples_out  device fp32 [B,members,C,H,W] or NULL: the blended image of every member
 *   tiles_out    device fp32 [members,B,ny*nx,C,th,tw] or NULL: the denoised tiles in run order -- slice m is the tiles_out of
 *                mi_denoise_tiled for member m (NULL: they live in the workspace).  At least one of the four outputs is given
 *   t_list .. noise_steps   as mi_denoise
 *   seed, sample_offset     as mi_denoise_seeded (sample_offset counts IMAGES)
 *   member_offset  member index of member 0 of this call, as in mi_denoise_ensemble
 *   pass_samples, flags     as mi_denoise_tiled
 * There is no unseeded form and no `seeded` switch: a deterministic sampler has no ensemble.  With a batch-invariant plan every tile output is a function of its crop and of (seed,
 * image, position, member) alone: not of B, members, pass_samples or the stream.
 * MI_EINVAL before any GPU work, with the limit named in mi_last_error: everything mi_denoise_tiled refuses; members < 1;
 * member_offset < 0; member_offset + members > 2^32 (4294967296); B * members * tiles > 2^31 - 1 (2147483647); no output pointer;
 * std_out with members < 2; any two of noisy, mean_out, std_out, samples_out, tiles_out overlapping.
 * The status word (mi_status) is cleared once per call and accumulates over the passes of every member.  Allocates nothing;
 * asynchronous. */
int mi_denoise_tiled_ensemble(mi_plan* plan, const float* noisy, float* mean_out, float* std_out, float* samples_out, float* tiles_out,
                              int B, int members, int H, int W, int th, int tw, int oy, int ox,
                              const int32_t* t_list, int n_iters,
                              const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                              uint64_t seed, int64_t sample_offset, int64_t member_offset, int pass_samples, int flags,
                              void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of workspace mi_denoise_tiled_ensemble needs: what mi_tiled_workspace_bytes answers for the same pass with
 * tiles_external != 0 (the sampler workspace of a pass of tiles + the pass's condition tiles; the passes of one member are those of
 * mi_denoise_tiled) + -- unless tiles_external != 0, i.e. tiles_out is given -- the tile outputs of every member,
 * members * B * ny*nx * C*th*tw * 4 bytes.  Host only, answered from the planner alone: it works before mi_unet_finalize too.
 * 0 on bad arguments (mi_last_error says which). */
size_t mi_tiled_ensemble_workspace_bytes(mi_plan* plan, int B, int members, int H, int W, int th, int tw, int oy, int ox,
                                         int pass_samples, int tiles_external);

/* The reduction of mi_denoise_tiled_ensemble on its own (no plan needed): tiles device fp32 [members][B][ny*nx][C][th][tw] ->
 * mean_out [B][C][H][W], std_out [B][C][H][W] or NULL (members >= 2) and samples_out [B][members][C][H][W] or NULL, the blended image
 * of every member.  One kernel; a thread owns one output element of one image.  THE ARITHMETIC (fixed, per pixel, independent of
 * the launch geometry, no atomics, no fused multiply-add) is the composition of the two specifications above, bit for bit:
 *   for m = 0 .. members-1:  v_m = the pixel of mi_tile_blend over tiles[m][b]  (a float: (float)(num / den))
 *   (mean, std) = the arithmetic of mi_ensemble_reduce over v_0 .. v_{members-1}, in index order
 * so the outputs equal mi_tile_blend of every member followed by mi_ensemble_reduce, and are the same bits with and without
 * samples_out (the v_m are formed again from the tiles for the deviations; nothing is read back).
 * MI_EINVAL: the cases of mi_tile_blend (geometry rules, C*H*W >= 2^32, B * tiles > 2^31 - 1, overlap > 46339) and of
 * mi_ensemble_reduce (B outside [1, 65535], members < 1, null tiles / mean_out, std_out with members < 2), and
 * B * members * tiles > 2^31 - 1.  tiles and the three outputs must not overlap. */
int mi_tile_blend_reduce(const float* tiles, int B, int members, int C, int H, int W, int th, int tw, int oy, int ox,
                         float* mean_out, float* std_out, float* samples_out, void* stream);

/* The quantile maps of an ensemble of tiled runs (no plan needed): tiles device fp32 [members][B][ny*nx][C][th][tw], as
 * mi_denoise_tiled_ensemble's tiles_out holds them, -> out [B][nq][C][H][W].  One kernel; a thread owns one output element of one
 * image with the addressing of mi_tile_blend_reduce.  THE ARITHMETIC (fixed, per pixel, no atomics, no fused multiply-add) is the
 * composition of two specifications above, bit for bit:
 *   for m = 0 .. members-1:  v_m = the pixel of mi_tile_blend over tiles[m][b]  (a float: (float)(num / den)), formed once
 *   out = the arithmetic of mi_ensemble_quantiles over v_0 .. v_{members-1}
 * so the output equals mi_tile_blend of every member followed by mi_ensemble_quantiles, and the blended members never exist in
 * memory.
 * MI_EINVAL: the cases of mi_tile_blend_reduce for the arguments the two share (geometry rules, C*H*W >= 2^32, B outside
 * [1, 65535], B * tiles and B * members * tiles > 2^31 - 1, overlap > 46339, members < 1) and of mi_ensemble_quantiles
 * (members > 64, nq outside [1, 8], null q / tiles / out, a level that is NaN or outside [0, 1]).  tiles and out must not overlap. */
int mi_tile_blend_quantiles(const float* tiles, int B, int members, int C, int H, int W, int th, int tw, int oy, int ox,
                            const double* q, int nq, float* out, void* stream);

/* GEOMETRIC SELF-ENSEMBLE ("x8 test-time augmentation"): the network runs on flipped and rotated copies of every image, every
 * output is turned back, and the per-pixel mean and spread over the views are returned -- for BOTH variants: it is the ensemble
 * of a deterministic (DDIM) sampler, whose std map shows where the output depends on the orientation.  (Not a reference call:
 * the reference denoises the image as given, DDIMModel.py:268-289.)
 * THE GEOMETRY (fixed).  A view code is g in 0..7, g = 4*t + 2*fy + fx; it acts on the last two axes of a [C,H,W] image, the same
 * way on every channel:
 *   view(x, g):    u = x with H and W swapped (u[i][j] = x[j][i]) if t, else x;
 *                  if fy: reverse the rows of u;  if fx: reverse the columns of u
 *   unview(y, g):  if fx: reverse the columns;  if fy: reverse the rows;  if t: swap the axes       (unview(view(x, g), g) == x)
 * Codes 0..3 are the identity, the left-right mirror, the up-down mirror and the half turn: they keep the shape and work for any
 * H, W the network takes.  Codes 4..7 are the transpose, the two quarter turns (5: clockwise, numpy.rot90(x, -1); 6: counter-
 * clockwise, numpy.rot90(x, 1)) and the anti-transpose: they turn H x W into W x H and are accepted ONLY when H == W, because a
 * pass never mixes image sizes.  A view list is 1 to 8 DISTINCT codes in the caller's order; the order is the order of the
 * members (samples_out, and the order of the sums of the mean).
 * THE GENERAL FORM of the transposing codes (t = 1), for any H x W plane -- used where a transposed image is acceptable, i.e. by
 * the TILED self-ensemble below; the calls of this section keep the H == W rule.  view(x, g) is Wv x Hv = W x H with
 *   view(x)[p][q] = x[fx ? H-1-q : q][fy ? W-1-p : p]
 * and its inverse is  unview(v)[y][x] = v[p][q]  with  p = fy ? W-1-x : x,  q = fx ? H-1-y : y.
 * For H == W == N this is the N x N form above (swap, then the reversals), entry for entry; the non-transposing codes are as above.
 *
 * mi_dihedral_views (no plan needed): dst device fp32 [n][C][Hv][Wv] <- view(images[v / n_views], views[v % n_views]) for the
 *   virtual samples v = v0 .. v0 + n - 1 of images [B][C][H][W] (image-major, v = b * n_views + k, as mi_denoise_ensemble numbers
 *   them): the fill of a pass on its own.  Bit copies.  n == 0: MI_OK.
 * mi_dihedral_reduce (no plan needed): views_out device fp32 [B][n_views][C][Hv][Wv], every view's output in ITS frame, ->
 *   mean_out [B][C][H][W], std_out (or NULL; n_views >= 2) and samples_out [B][n_views][C][H][W] (or NULL), the ALIGNED members
 *   x_k = unview(views_out[b][k], views[k]).  THE ARITHMETIC (fixed, per pixel) is mi_ensemble_reduce's over x_0 .. x_{n_views-1}
 *   in list order: the result equals unview per view followed by mi_ensemble_reduce, bit for bit, with or without samples_out.
 *   The aligned members are never stored unless samples_out is given.  At least one output; views_out and the outputs must not overlap.
 * mi_dihedral_quantiles (no plan needed): the same gather, then THE ARITHMETIC of mi_ensemble_quantiles over the aligned members:
 *   out [B][nq][C][H][W] equals mi_ensemble_quantiles of them, bit for bit.
 * MI_EINVAL of the three, before any GPU work, in this order: C < 1; a bad shape or C*H*W >= 2^32; n_views outside [1, 8]; null
 *   views; a code outside [0, 7]; a repeated code; a transposing code with H != W; B outside [1, 65535]; then per call -- views:
 *   v0 < 0, n < 0, n > 65535 or v0 + n > B * n_views; reduce: no output pointer, std_out with one view; quantiles: the level rules of
 *   mi_ensemble_quantiles -- and last a null data pointer. */
int mi_dihedral_views(const float* images, int B, int C, int H, int W, const int32_t* views, int n_views,
                      int v0, int n, float* dst, void* stream);
int mi_dihedral_reduce(const float* views_out, int B, int C, int H, int W, const int32_t* views, int n_views,
                       float* mean_out, float* std_out, float* samples_out, void* stream);
int mi_dihedral_quantiles(const float* views_out, int B, int C, int H, int W, const int32_t* views, int n_views,
                          const double* q, int nq, float* out, void* stream);

/* mi_denoise_ensemble with the views of an image in the place of its draws.  The B * n_views virtual samples (v = b * n_views + k:
 * view k of image b) run through mi_denoise's sampler loop in passes of at most pass_samples consecutive virtual samples -- the
 * fill of a pass is mi_dihedral_views, each pass is split over two streams as a mi_denoise batch of that size is -- and ONE
 * mi_dihedral_reduce launch follows the last pass.
 *   noisy        device fp32 [B,C,H,W]; never written
 *   mean_out     device fp32 [B,C,H,W] or NULL
 *   std_out      device fp32 [B,C,H,W] or NULL; needs n_views >= 2
 *   samples_out  device fp32 [B,n_views,C,H,W] or NULL: the ALIGNED members, unview of every view's output
 *   views        HOST int32[n_views]
 *   seeded       0: no noise term -- the DDIM variant, or cddpm's noise-free use; nothing is drawn.  != 0: view k of image b draws
 *                the step noise of (seed, sample_offset + b, member word member_offset + k) with the counter word c0 the pixel's
 *                index IN THE VIEW'S FRAME: view k is mi_denoise_seeded -- as member member_offset + k, mi_denoise_ensemble's
 *                single-member form -- of the turned image view(noisy[b], views[k]), bit for bit with a batch-invariant plan
 *   pass_samples, flags, t_list .. noise_steps   as mi_denoise_ensemble
 * The view-frame outputs ALWAYS live in the workspace (unview of a transposing view cannot run in place), so the workspace does
 * not shrink when samples_out is given.  They are its LAST B * n_views * C*H*W * 4 bytes, counted from the size
 * mi_self_ensemble_workspace_bytes answers, laid out [B][n_views][C][Hv][Wv]: after the call a caller may hand that address to
 * mi_dihedral_quantiles (or mi_dihedral_reduce) on the same stream.
 * MI_EINVAL before any GPU work, the rule named in mi_last_error, in this order: null plan; n_views outside [1, 8]; null views; a
 * code outside [0, 7]; a repeated code; a transposing code with H != W; member_offset < 0; member_offset + n_views > 2^32;
 * pass_samples < 1; B outside [1, 65535] or B * n_views > 2^31 - 1; sample_offset < 0; C*H*W >= 2^32; no output pointer; std_out
 * with one view; any two of noisy, mean_out, std_out, samples_out overlapping.  (sample_offset and member_offset are judged when
 * seeded == 0 too.)  Then, as every batched call: the plan's state, the workspace, null noisy, the schedule, the device.
 * The status word (mi_status) is cleared once per call and accumulates over the passes.  Allocates nothing; asynchronous. */
int mi_denoise_self_ensemble(mi_plan* plan, const float* noisy, float* mean_out, float* std_out, float* samples_out,
                             int B, int H, int W, const int32_t* views, int n_views,
                             const int32_t* t_list, int n_iters,
                             const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                             int seeded, uint64_t seed, int64_t sample_offset, int64_t member_offset, int pass_samples, int flags,
                             void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of workspace mi_denoise_self_ensemble needs: mi_ensemble_workspace_bytes(plan, B, n_views, H, W, pass_samples, 0) -- the
 * sampler workspace of a pass + the pass's condition views + the view outputs, B * n_views * C*H*W * 4 bytes.  samples_external is
 * accepted for symmetry with the other queries and IGNORED: the view outputs stay in the workspace whether or not samples_out is
 * given.  Host only, answered from the planner alone: it works before mi_unet_finalize too.  0 on bad arguments (mi_last_error). */
size_t mi_self_ensemble_workspace_bytes(mi_plan* plan, int B, int n_views, int H, int W, int pass_samples, int samples_external);

/* THE DDIM UPDATE: a stride-aware update rule for the sampler loop (Song, Meng, Ermon: Denoising Diffusion Implicit Models,
 * eq. 12 and 16), opt-in.  The reference's update, x <- clamp(c1 * (x - c2 * eps) + c3 * noise, 0, 1), is the one-step ancestral mean
 * for t -> t-1 whatever the list; on a strided list (t, t-6, t-12, ...) every iteration still removes one step's share of the
 * noise.  This rule predicts x0 from eps, optionally clips it to the image range, and re-noises it to the NEXT timestep of the
 * list.  Not a reference rule: the default (NULL, or kind MI_UPDATE_REFERENCE) stays the reference's, with the reference's bits.
 * THE SPECIFICATION (fixed).  The list t_0 > t_1 > ... > t_{n-1} is strictly decreasing.  Iteration i has
 * A = alpha_hat[t_i] and P = alpha_hat[t_{i+1}], P = 1 for the last iteration; 0 < A < P <= 1.
 * Host, in double precision from the caller's fp32 table, every operation rounded on its own, each value rounded once to fp32:
 *   sigma = eta * sqrt((1-P)/(1-A)) * sqrt(1 - A/P)             (products left to right)
 *   k0 = 1/sqrt(A)    k1 = sqrt(1-A)    r0 = sqrt(A)    r1 = 1/sqrt(1-A)
 *   a  = sqrt(P)      b  = sqrt(max(0, (1-P) - sigma*sigma))     s = 2*sigma
 * s carries the factor 2 because the step-noise convention stays what it is: the tensor argument and the seeded generator both
 * deliver n = 0.5 * z, and neither they nor mi_step_noise_fill change.  The last row is a = 1, b = 0, s = 0; eta = 0 gives s = 0
 * in every row (the deterministic sampler), eta = 1 on the stride-1 list the ancestral sampler's variance.
 * Device, per element, fp32, every operation rounded on its own (no fused multiply-add anywhere in this update; fmin / fmax as
 * C's fminf / fmaxf), in this order:
 *   e  = flags & MI_CLAMP_EPS ? min(max(eps, -5), 5) : eps
 *   x0 = k0 * (x - k1*e)
 *   if clip_x0:  c = min(max(x0, 0), 1);  if c != x0: e = (x - r0*c) * r1;  x0 = c
 *                (eps re-derived, so that x_prev stays on the trajectory towards the clipped image)
 *   xn = a*x0 + b*e
 *   if s > 0 and the call has a noise source:  xn = xn + s*n       (n: step_noise[i] or the seeded draw of iteration i)
 *   if i == n-1:  xn = min(max(xn, 0), 1)       (the call returns an image in [0, 1] like every other call)
 * Intermediate x is NOT clamped to [0, 1] under this rule: x_t = sqrt(A) x0 + sqrt(1-A) eps leaves [0, 1] by design, and a clamp
 * would take it off the trajectory the next iteration's x0 prediction assumes.  Nothing is drawn or read when s == 0 -- every
 * iteration at eta = 0, always the last one.  tests/ddim_update_reference.py restates host and device in numpy, bit for bit.
 * The start state stays the noisy image itself, as in the reference. */
#define MI_UPDATE_REFERENCE 0
#define MI_UPDATE_DDIM      1
typedef struct mi_update_rule {
    int32_t kind;      /* MI_UPDATE_* */
    double  eta;       /* MI_UPDATE_DDIM: finite, in [0, 1] */
    int32_t clip_x0;   /* MI_UPDATE_DDIM: != 0 clips the predicted image to [0, 1] */
} mi_update_rule;

/* The coefficient table of the rule above, host only (no plan, no GPU): out HOST fp32 [n_iters][7] <- (k0, k1, r0, r1, a, b, s) of
 * every iteration -- the values the *_rule calls below pass to the update kernel.
 * MI_EINVAL: eta outside [0, 1] or NaN; a null argument; noise_steps < 1; a timestep outside [0, noise_steps); a list that is not
 * strictly decreasing; a table with alpha_hat[t_i] outside (0, alpha_hat[t_{i+1}]). */
int mi_ddim_coefficients(const int32_t* t_list, int n_iters, const float* alpha_hat, int noise_steps, double eta, float* out);

/* mi_denoise and mi_denoise_seeded in one signature (step_noise, or seeded != 0 with seed and sample_offset; both: MI_EINVAL), plus
 * `rule`.  rule == NULL or kind MI_UPDATE_REFERENCE: those two calls, bit for bit.  MI_UPDATE_DDIM: the update above in the place
 * of the reference's; everything else -- the forward, the two-stream split, the seeded generator's counter words, the workspace
 * (mi_workspace_bytes: the rule needs no memory) -- is the same.  The rule's own MI_EINVAL cases (mi_ddim_coefficients) are judged
 * first, before the plan's state and before any GPU work.  With eta > 0 the call takes a noise source for EITHER variant; without
 * one the term is left out. */
int mi_denoise_rule(mi_plan* plan, const float* noisy, float* x_out, int B, int H, int W,
                    const int32_t* t_list, int n_iters,
                    const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                    const float* step_noise, int seeded, uint64_t seed, int64_t sample_offset, int flags,
                    const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream);

/* mi_denoise_ensemble plus `rule`: every pass runs the loop under the rule.  NULL / reference: mi_denoise_ensemble bit for bit.
 * With MI_UPDATE_DDIM and eta > 0 the DDIM variant has an ensemble too (eta == 0 draws nothing: all members are equal; the host
 * shims refuse it).  Workspace: mi_ensemble_workspace_bytes. */
int mi_denoise_ensemble_rule(mi_plan* plan, const float* noisy, float* mean_out, float* std_out, float* samples_out,
                             int B, int members, int H, int W,
                             const int32_t* t_list, int n_iters,
                             const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                             uint64_t seed, int64_t sample_offset, int64_t member_offset, int pass_samples, int flags,
                             const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream);

/* mi_denoise_tiled plus `rule`, likewise.  Workspace: mi_tiled_workspace_bytes.
 * The per-slot loop runs the rule through mi_denoise_slots_rule below (mi_denoise_slots and mi_denoise_slots_virtual themselves keep
 * the reference's).  NOT BUILT: mi_denoise_tiled_ensemble and mi_denoise_self_ensemble (plumbing only) keep the reference's rule. */
int mi_denoise_tiled_rule(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out,
                          int B, int H, int W, int th, int tw, int oy, int ox,
                          const int32_t* t_list, int n_iters,
                          const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                          int seeded, uint64_t seed, int64_t sample_offset, int pass_samples, int flags,
                          const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream);

/* THE DPMPP2M UPDATE: a second-order multistep update for the sampler loop (Lu et al. 2022, DPM-Solver++(2M)) with its
 * extrapolation weight bounded, opt-in.  The DDIM update above is first order and throws away the predicted image x0 that every
 * iteration computes; this rule keeps the previous iteration's and extrapolates.  It costs no network evaluation and one
 * image-sized buffer, which the caller owns -- and which, given one slot per iteration, is the trajectory of predicted images.
 * Since x = sqrt(A) x0 + sqrt(1-A) eps, the 2M step is the DDIM (eta = 0) step plus one term:
 *   x_next = a*x0 + b*e + g*(x0 - x0_prev)
 * THE SPECIFICATION (fixed).  List, A and P as under THE DDIM UPDATE.
 * Host, for the rows 0 < i < n-1, in double precision from the caller's fp32 table, every operation rounded on its own:
 *   lambda(X) = 0.5 * log(X / (1-X))              (half the log-SNR)
 *   h_i = lambda(P) - lambda(A)        r = h_{i-1} / h_i
 *   emh = sqrt(((1-P)/(1-A)) * (A/P))             (= e^{-h_i}, without exp)
 *   g   = sqrt(P) * (1 - emh) / (2 * max(r, 1))   rounded once to fp32
 * g = 0 on the first row (no history) and on the last (P = 1: h is infinite).  The textbook weight is 1/(2r); max(r, 1) bounds it
 * at its uniform-step value 1/2.  The reference's schedule jumps in log-SNR at t = 0 (h = 2.27 after 0.64 on the 9-entry list), r
 * falls to 0.28 and the unbounded weight 1.8 makes the rule WORSE than DDIM on the short lists; bounded it is better on every one
 * (the Gaussian check).  k0, k1, r0, r1, a, b are the DDIM table's at eta = 0, bit for bit.
 * Device, per element, fp32, every operation rounded on its own (no fused multiply-add), in this order: the DDIM update's
 *   e, x0 (clipped when clip_x0, eps re-derived), xn = a*x0 + b*e            -- the same text
 *   if g != 0:   xn = xn + g * (x0 - x0_prev)         (x0, x0_prev: the clipped predictions)
 *   if i == n-1: xn = min(max(xn, 0), 1)
 *   x0 is stored
 * g is launch-uniform; nothing of the history is read when g == 0.  Deterministic: there is no eta and no noise term, for either
 * variant.  Start state and list rules as under THE DDIM UPDATE.  tests/dpm_update_reference.py restates host and device in numpy. */
#define MI_UPDATE_DPMPP2M   2

/* The coefficient table of the rule above, host only: out HOST fp32 [n_iters][8] <- (k0, k1, r0, r1, a, b, s, g).  The first seven
 * columns are mi_ddim_coefficients at eta = 0, bit for bit (s is 0).  MI_EINVAL as mi_ddim_coefficients. */
int mi_dpm_coefficients(const int32_t* t_list, int n_iters, const float* alpha_hat, int noise_steps, float* out);

/* mi_denoise under the rule above.  x0_buf: the caller's DEVICE buffer fp32 [x0_slots, B, C, H, W] of predicted images, overlapping
 * neither noisy nor x_out.  x0_slots == 1: the history, read and written in place (every thread reads its own element before it
 * writes it); it ends as the last iteration's prediction.  x0_slots == n_iters: the trajectory -- iteration i reads slot i-1 and
 * writes slot i.  Any other x0_slots is MI_EINVAL.  x_out is the same bits either way.  The buffer is never read before it is
 * written: it needs no initialisation.  clip_x0 != 0 clips the predicted image to [0, 1] (then the last slot equals x_out).
 * Everything else -- the forward, the two-stream split (each sub-batch owns its images of every slot), the workspace
 * (mi_workspace_bytes: the rule needs none) -- is mi_denoise's.  The rule's MI_EINVAL cases are judged first, as in mi_denoise_rule.
 * MI_UPDATE_DPMPP2M handed to the *_rule calls above is MI_EINVAL: they have no buffer. */
int mi_denoise_dpm(mi_plan* plan, const float* noisy, float* x_out, float* x0_buf, int x0_slots, int B, int H, int W,
                   const int32_t* t_list, int n_iters,
                   const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                   int flags, int clip_x0, void* workspace, size_t workspace_bytes, void* stream);

/* mi_denoise_tiled under the rule above (no seed: deterministic).  x0_hist: DEVICE fp32 [pass_samples, C, th, tw], the in-place
 * history of whichever pass runs, reused by every pass; there is no trajectory for tiles.  Workspace: mi_tiled_workspace_bytes.
 * The per-slot loop under this rule is mi_denoise_slots_rule below.
 * NOT BUILT under this rule: ensembles of any kind (nothing is drawn), an SDE (eta > 0) form, a third order. */
int mi_denoise_tiled_dpm(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out, float* x0_hist,
                         int B, int H, int W, int th, int tw, int oy, int ox,
                         const int32_t* t_list, int n_iters,
                         const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                         int pass_samples, int flags, int clip_x0, void* workspace, size_t workspace_bytes, void* stream);

/* One row of both tables from a timestep and its NEIGHBOURS in a list, host only (no plan, no GPU): out HOST fp32 [8] <-
 * (k0, k1, r0, r1, a, b, s, g) of the iteration at t whose list has t_before in front of it and t_after behind it; -1 = none.
 * t_before = -1 is a list's first row (g = 0), t_after = -1 its last (P = 1: a = 1, b = 0, s = 0, g = 0).  Columns 0 .. 6 are the
 * row of mi_ddim_coefficients at `eta`, column 7 the g of mi_dpm_coefficients, bit for bit: the list forms ask this function.
 * MI_EINVAL as mi_ddim_coefficients, applied to the triple: eta; a null argument; noise_steps < 1; t outside [0, noise_steps),
 * a neighbour outside [-1, noise_steps); a triple that is not strictly decreasing; alpha_hat outside the rule on either step. */
int mi_update_row(int32_t t_before, int32_t t, int32_t t_after, const float* alpha_hat, int noise_steps, double eta, float out[8]);

/* TILED SELF-ENSEMBLE: the flip / rotate views of images of ANY size >= the tile, at their own size -- the cell that was missing
 * between mi_denoise_self_ensemble (one network-sized image) and mi_denoise_tiled_ensemble (seeded draws, tiled).  It is the
 * ensemble a deterministic (DDIM) model has for a full-resolution image.
 * A VIEW'S TILES ARE THE TILES OF THE VIEWED IMAGE.  View k of image b is the Hv x Wv image view(noisy[b], g_k) (THE GEOMETRY
 * above, general form).  It is cut by THE GEOMETRY of tiled denoising in the view's OWN frame -- the tile counts and origins of
 * mi_tile_geometry for (Hv, th, oy) and (Wv, tw, ox) -- and its tiles are numbered ky * nx_v + kx there.  This is NOT the view of
 * every tile of the un-viewed image: the origin formula rounds down, so a mirrored image's tiles sit elsewhere whenever
 * (L - T) % (n - 1) != 0 (L = 41, T = 16, O = 4: origins 0, 8, 16, 25, whose mirror is 0, 9, 17, 25).  The definition chosen makes
 * every member the composition of two existing public calls (below).
 * TRANSPOSING CODES (4 .. 7) are accepted iff th == tw and oy == ox: then the W x H frame has nx * ny tiles of the same shape, the
 * tile count K = ny * nx is the same in both frames and the storage [n_views][B][K][C][th][tw] is rectangular.  H == W is NOT
 * required: a transposed image is still cut into th x tw tiles.
 *
 * mi_tile_blend_unview_reduce (no plan needed): tiles device fp32 [n_views][B][K][C][th][tw], the tile outputs of every view in
 *   that view's frame, in run order -> mean_out [B][C][H][W], std_out (or NULL; n_views >= 2) and samples_out
 *   [B][n_views][C][H][W] (or NULL), the aligned blended members, all in the IMAGE's frame (H, W, th, tw, oy, ox: the un-viewed
 *   image's).  One kernel.  THE ARITHMETIC (fixed, per output pixel (c, y, x), no atomics, no fused multiply-add, nothing depends
 *   on the launch geometry) is the composition of two specifications above, bit for bit:
 *     for k in list order:  v_k = the pixel (c, p_k, q_k) of mi_tile_blend over tiles[k][b] with the geometry (Hv, Wv, th, tw, oy,
 *       ox) of view k's frame -- (p_k, q_k) = (y, x) mapped by the view (non-transposing: p = fy ? H-1-y : y, q = fx ? W-1-x : x;
 *       transposing: p = fy ? W-1-x : x, q = fx ? H-1-y : y), the covering tiles walked in ascending (ky, kx) of THAT frame
 *     (mean, std) = the arithmetic of mi_ensemble_reduce over v_0 .. v_{n_views-1}
 *   so the outputs equal mi_tile_blend per view, unview, mi_ensemble_reduce, and are the same bits with and without samples_out.
 * mi_tile_blend_unview_quantiles (no plan needed): the same gather, every v_k formed once, then THE ARITHMETIC of
 *   mi_ensemble_quantiles over them: out [B][nq][C][H][W].  The aligned members never exist in memory.
 * MI_EINVAL of the two, before any GPU work, in this order: the cases of mi_tile_blend (C < 1, the geometry rules, overlap > 46339,
 *   B * tiles > 2^31 - 1, C*H*W >= 2^32); n_views outside [1, 8]; null views; a code outside [0, 7]; a repeated code; a transposing
 *   code with th != tw or oy != ox; B outside [1, 65535]; B * n_views * tiles > 2^31 - 1; then per call -- reduce: no output pointer,
 *   std_out with one view; quantiles: the level rules of mi_ensemble_quantiles -- and last a null data pointer.  tiles and the
 *   outputs must not overlap. */
int mi_tile_blend_unview_reduce(const float* tiles, int B, int C, int H, int W, int th, int tw, int oy, int ox,
                                const int32_t* views, int n_views, float* mean_out, float* std_out, float* samples_out, void* stream);
int mi_tile_blend_unview_quantiles(const float* tiles, int B, int C, int H, int W, int th, int tw, int oy, int ox,
                                   const int32_t* views, int n_views, const double* q, int nq, float* out, void* stream);

/* mi_denoise_tiled_ensemble with the views of an image in the place of its draws.  Views are the OUTER loop: round k makes
 * view(noisy, g_k) of the whole batch (a copy in the workspace; the identity is read in place) and runs its B * K (image, tile)
 * virtual samples exactly as mi_denoise_tiled runs them on that viewed batch -- extract (bit for bit the slices of the viewed
 * image), then the sampler loop, in passes of at most pass_samples, each pass split over two streams as a mi_denoise batch of
 * that size is (MI_NO_SPLIT honoured).  A pass never spans two views.  ONE mi_tile_blend_unview_reduce launch follows the last
 * pass of the last view.
 *   noisy        device fp32 [B,C,H,W]; never written
 *   mean_out     device fp32 [B,C,H,W] or NULL
 *   std_out      device fp32 [B,C,H,W] or NULL; needs n_views >= 2
 *   samples_out  device fp32 [B,n_views,C,H,W] or NULL: the ALIGNED blended members
 *   tiles_out    device fp32 [n_views,B,K,C,th,tw] or NULL: the denoised tiles in run order, view k's in ITS frame -- what
 *                mi_tile_blend_unview_quantiles takes (NULL: they live in the workspace).  At least one of the four is given
 *   views        HOST int32[n_views]
 *   seeded       0: nothing is drawn.  != 0: view k draws the member word member_offset + k, with the counter word c0 the pixel's
 *                index in the WHOLE VIEWED image (mi_denoise_tiled's rule in the view's frame, mi_denoise_self_ensemble's member rule)
 *   rule         NULL or MI_UPDATE_REFERENCE: the reference's update.  MI_UPDATE_DDIM (any eta; with eta > 0 the term is drawn when
 *                seeded != 0): as mi_denoise_tiled_rule.  MI_UPDATE_DPMPP2M: refused by name (the call takes no history buffer)
 *   the rest     as mi_denoise_tiled_ensemble
 * WHAT THE CALL IS, each statement bit for bit:
 *   unseeded (DDIM, or any plan with seeded == 0): member k = unview(image_out of mi_denoise_tiled on view(noisy, g_k), g_k) at the
 *     same pass_samples (under `rule`: of mi_denoise_tiled_rule);
 *   seeded: member k = the single sample of mi_denoise_tiled_ensemble on view(noisy, g_k) with members = 1 and member_offset =
 *     member_offset + k, turned back;
 *   views = [0] at member_offset = 0 IS mi_denoise_tiled / mi_denoise_tiled_rule (mean_out = image_out, tiles_out = tiles_out);
 *   with a batch-invariant plan every tile of every view is mi_denoise of its crop of view(x) -- with the crop of
 *     mi_step_noise_fill_member for the viewed shape, image sample_offset + b, member member_offset + k, where seeded -- whatever
 *     the pass size.
 * MI_EINVAL before any GPU work, the rule named in mi_last_error, in this order: the update rule's own cases (MI_UPDATE_DPMPP2M by
 * name, then those of mi_ddim_coefficients); null plan; n_views outside [1, 8]; null views; a code outside [0, 7]; a repeated code;
 * a transposing code with th != tw or oy != ox; then everything mi_denoise_tiled_ensemble refuses with members = n_views, in its
 * order; B > 65535; no output pointer; std_out with one view; any two of noisy, mean_out, std_out, samples_out, tiles_out
 * overlapping.  Then, as every batched call: the plan's state, the workspace, null noisy, the schedule, the device.
 * The status word (mi_status) is cleared once per call and accumulates over the passes of every view.  Allocates nothing;
 * asynchronous.  NOT BUILT: a session ticket for this call, MI_UPDATE_DPMPP2M, and the rule for mi_denoise_tiled_ensemble /
 * mi_denoise_self_ensemble, which keep the reference's update. */
int mi_denoise_tiled_self_ensemble(mi_plan* plan, const float* noisy, float* mean_out, float* std_out, float* samples_out, float* tiles_out,
                                   int B, int H, int W, int th, int tw, int oy, int ox, const int32_t* views, int n_views,
                                   const int32_t* t_list, int n_iters,
                                   const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                                   int seeded, uint64_t seed, int64_t sample_offset, int64_t member_offset, int pass_samples, int flags,
                                   const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of workspace mi_denoise_tiled_self_ensemble needs, THE SUM OF: what mi_tiled_workspace_bytes answers for the same pass with
 * tiles_external != 0 (the sampler workspace of a pass of tiles + the pass's condition tiles); the viewed copy of the batch of the
 * round that runs, B * C*H*W * 4 bytes rounded up to a multiple of 256 (counted whatever the list, so the size depends on the
 * NUMBER of views alone); and -- unless tiles_external != 0, i.e. tiles_out is given -- the tile outputs of every view,
 * n_views * B * K * C*th*tw * 4 bytes, the LAST bytes of the workspace.  Host only, answered from the planner alone: it works
 * before mi_unet_finalize too.  0 on bad arguments (mi_last_error says which). */
size_t mi_tiled_self_ensemble_workspace_bytes(mi_plan* plan, int B, int n_views, int H, int W, int th, int tw, int oy, int ox,
                                              int pass_samples, int tiles_external);

/* CONTINUOUS BATCHING UNDER A RULE: mi_denoise_slots_virtual plus `rule`, every slot at its own place in its own list.
 * rule == NULL or kind MI_UPDATE_REFERENCE: mi_denoise_slots_virtual, bit for bit, the same launches; t_before, t_after and x0_hist
 * must then be NULL.  MI_UPDATE_DDIM (x0_hist NULL) and MI_UPDATE_DPMPP2M (x0_hist required; seeded and step_noise refused: the
 * rule is deterministic) run THE DDIM UPDATE / THE DPMPP2M UPDATE per slot: the row of slot b in row i is mi_update_row of
 *   previous = t_rows[i-1][b], or t_before[b] in the call's first row
 *   next     = t_rows[i+1][b], or t_after[b] in the call's last row; -1 there (or an idle row) means the slot's list ends with
 *              this row: it is the list's LAST row, a = 1, and the result is clamped to [0, 1]
 * so a list cut into calls anywhere -- a session's call boundaries -- gives the coefficients, and with a batch-invariant plan the
 * bits, of the list run whole; a uniform table with x preset to the condition gives mi_denoise_rule's / mi_denoise_dpm's bits at
 * the same B.
 *   t_before, t_after  HOST int32 [B] or NULL (all -1)
 *   x0_hist            DEVICE fp32 [B,C,H,W], MI_UPDATE_DPMPP2M only: slot b's previous predicted image, read (where g != 0) and
 *                      written (every active slot) in place, each thread its own element; an idle slot's keeps its bits.  It
 *                      travels with the slot: a caller that moves a slot's x moves its x0_hist.  Never read before it is written
 *                      (a list's first row has g = 0): no initialisation.  Overlaps neither cond nor x
 * The noise term s * n is added where the row's s > 0 and the call has a noise source, drawn with the slot's counter words exactly
 * as mi_denoise_slots_virtual draws.  Sub-batches, phase offset, join, status word: as mi_denoise_slots; sub-batch h takes its
 * columns of x0_hist too.  The records are 64 bytes a slot and live where mi_denoise_slots' 48-byte records live: the region is
 * sized for the larger, so mi_workspace_bytes grows by 16 bytes per sample (before its 256-byte rounding).
 * MI_EINVAL, judged before the plan's state and before any GPU work (mi_last_error names the argument): the kinds' rules above,
 * first; every rule of mi_denoise_slots_virtual; t_before / t_after outside [-1, noise_steps); a column whose sequence
 * (t_before, active rows, t_after) is not strictly decreasing or breaks mi_ddim_coefficients' alpha_hat rule on a step;
 * t_after[b] >= 0 for a slot that went idle inside the call; x0_hist overlapping x or cond. */
int mi_denoise_slots_rule(mi_plan* plan, const float* cond, float* x, int B, int H, int W,
                          const int32_t* t_rows, int n_rows, const int32_t* iter_base, const int64_t* sample_index,
                          const int64_t* member, const uint32_t* frame,
                          const int32_t* t_before, const int32_t* t_after, float* x0_hist,
                          const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                          const float* step_noise, int seeded, uint64_t seed, int flags,
                          const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream);

/* TILED DENOISING, FUSED: the overlapping tiles agree after EVERY step.  mi_denoise_tiled runs the whole sampler loop on each tile
 * alone and cross-fades what the tiles ended up with; the network has attention, so two tiles make different global decisions about
 * the strip they share, and the ramp only hides it.  Here the steps are the outer loop and the overlapping STATES are fused after
 * each one (MultiDiffusion / Mixture of Diffusers), so every tile enters the next forward with the same values wherever it shares
 * pixels with a neighbour.  The seeded step noise belongs to the image (mi_denoise_tiled: `seeded`), so overlapping tiles draw the
 * same noise at the same pixel and averaging their states does not shrink the noise variance in the overlaps.
 *
 * THE CONSENSUS (fixed; no plan needed).  tiles device fp32 [B][ny*nx][C][th][tw], IN PLACE; image_out device fp32 [B][C][H][W] or
 * NULL.  For every image pixel
 *   v = the value of mi_tile_blend over the tiles that cover it: the same walk in ascending (ky, kx), the same double arithmetic
 *       with every operation rounded on its own and no fused multiply-add, one rounding to fp32 (THE ARITHMETIC above)
 *   v is written to that pixel's element in EVERY covering tile, and to image_out if one is given.
 * By definition the tiles afterwards are mi_tile_extract(mi_tile_blend(tiles)) and image_out is mi_tile_blend(tiles), bit for bit,
 * whatever the launch geometry, the alignment of the pointers or the load width the kernel picks; the call is idempotent.  A pixel
 * under one tile keeps its value as mi_tile_blend keeps it.  One launch, one pass, no image-sized temporary: per pixel `cover`
 * reads and `cover` (+ 1) writes.  In place is safe because a tile element lies over exactly one pixel and the thread that owns a
 * pixel reads all of its covering elements before it writes any.  No atomics.
 * MI_EINVAL before any GPU work: everything mi_tile_blend refuses (the geometry rules, C*H*W >= 2^32, B * tiles > 2^31 - 1,
 * overlap > 46339, null tiles), and an image_out that overlaps tiles. */
int mi_tile_consensus(float* tiles, int B, int C, int H, int W, int th, int tw, int oy, int ox, float* image_out /* or NULL */, void* stream);

/* The step-outer tiled sampler.  Arguments as mi_denoise_tiled_rule, plus x0_hist: DEVICE fp32 [B*ny*nx, C, th, tw], every tile's own
 * previous predicted image -- required under MI_UPDATE_DPMPP2M (which this call takes, with seeded == 0), NULL under every other rule.
 * THE SPECIFICATION is this composition of public calls, which the call equals BIT FOR BIT at the same pass_samples and flags:
 *   cond[v] = tile v of noisy (mi_tile_extract);  x[v] = cond[v]                      v = b * (ny*nx) + k
 *   for i in 0 .. n_iters-1:
 *       for each pass of pass_samples consecutive v (the last one may be shorter):
 *           ONE ROW of mi_denoise_slots_rule on (cond[pass], x[pass]):
 *               t_rows = t_list[i] in every column, iter_base = i, sample_index = sample_offset + b(v), member = 0,
 *               frame = (W, H*W, y0*W + x0) of the tile when seeded != 0 (else NULL),
 *               t_before = t_list[i-1] or -1, t_after = t_list[i+1] or -1 (NULL under the reference's update),
 *               x0_hist[pass] under MI_UPDATE_DPMPP2M, the caller's rule and flags
 *       mi_tile_consensus(x, ...)          -- the one after the last step also writes image_out
 *   tiles_out = x
 * With a batch-invariant plan the result does not depend on pass_samples at all.  Only x is fused: the x0 history is a tile's own
 * prediction.  Under the reference's update x is the clamped image state, under MI_UPDATE_DDIM and MI_UPDATE_DPMPP2M the unclamped
 * x_t; the consensus is linear and convex either way, so a fused state stays inside the range of the states it fuses.  One tile that
 * is the image is mi_denoise_rule / mi_denoise_dpm of it.  n_iters == 0 behaves as mi_denoise_tiled does (the tiles are the crops,
 * image_out their blend).
 * As mi_denoise_tiled: every rule is judged before the first launch; the plan's side streams are held over the call; the status
 * word (mi_status) is cleared once and accumulates over all (step, pass) runs; every run joins its side streams -- once per
 * (step, pass), where mi_denoise_tiled joins once per pass --; no device memory is allocated; the host never waits.
 * MI_EINVAL before any GPU work: everything mi_denoise_tiled_rule refuses; MI_UPDATE_DPMPP2M with seeded != 0 or without x0_hist;
 * x0_hist under any other rule; any two of noisy, image_out, tiles_out, x0_hist overlapping.
 * NOT BUILT: fused tiled ensembles and self-ensembles, fused tickets of a session, fusing every n-th step or a range of steps,
 * fusing the x0 history, a trajectory. */
int mi_denoise_tiled_fused(mi_plan* plan, const float* noisy, float* image_out, float* tiles_out, float* x0_hist,
                           int B, int H, int W, int th, int tw, int oy, int ox,
                           const int32_t* t_list, int n_iters,
                           const float* beta, const float* alpha, const float* alpha_hat, int noise_steps,
                           int seeded, uint64_t seed, int64_t sample_offset, int pass_samples, int flags,
                           const mi_update_rule* rule, void* workspace, size_t workspace_bytes, void* stream);

/* Bytes of workspace mi_denoise_tiled_fused needs, THE SUM OF: the sampler workspace of a pass of tiles (as mi_tiled_workspace_bytes
 * counts it); the condition tiles of ALL B * ny*nx virtual samples, rounded up to 256 bytes -- they are extracted once and kept for
 * the whole call, since every step reads them again; and -- unless tiles_external != 0, i.e. tiles_out is given -- the tile states,
 * B * ny*nx * C*th*tw * 4 bytes.  Host only, answered from the planner alone (it works before mi_unet_finalize); 0 + mi_last_error
 * for arguments the call would refuse. */
size_t mi_tiled_fused_workspace_bytes(mi_plan* plan, int B, int H, int W, int th, int tw, int oy, int ox, int pass_samples, int tiles_external);

/* Status of the last mi_unet_forward / mi_denoise call that used `workspace` (its first word; the calls clear it when they
 * start).  SYNCHRONISES `stream` (one 4-byte device-to-host copy).  Returns MI_OK with *flags == 0, or MI_ERANGE with the
 * MI_STATUS_* bits in *flags: the kernels never turn a NaN / Inf activation or an operand beyond the split-fp16 range into
 * finite garbage silently -- the output is NaN where the reference's is, and this call says why.  (The reference itself
 * reports nothing: torch propagates NaN, DDIMModel.py:219-289.) */
int mi_status(const void* workspace, void* stream, int* flags);

/* Debug/test hook: after a forward call, copies the output of the named top-level module
 * (e.g. "downs.3", "mid_attn", "ups.6") from the workspace to `dst` (device fp32, NCHW
 * [B,C,h,w]); returns its C,h,w.  `dst` may be NULL to query the shape only. */
int mi_debug_fetch(mi_plan* plan, const char* module_name, int B, int H, int W,
                   const void* workspace, float* dst, int* C, int* h, int* w, void* stream);

/* Debug/test hook, host only (no GPU call): the key split the split-fp16 attention kernel uses for N keys (pixels of
 * the attention level) when the execution program holds B samples: number of splits and 32-key tiles per split.
 * Every split owns at least one tile for every N >= 1 (tests sweep it). */
int mi_debug_attention_split(int N, int B, int* ksplit, int* tiles_per_split);

/* Debug/test hook, host only (no GPU call, no finalize needed): the execution program the planner builds for (B, H, W) as
 * text, one line per kernel launch: kernel instantiation, tile, grid, persistent workgroups per sample, weight-ring depth and
 * DMA pieces per wave, folded res_conv steps, attention key split, LDS bytes.  side_by_side != 0: the sub-batch program the
 * two-stream mi_denoise runs (the reference has no counterpart: its graph is fixed, DDIMModel.py:219-248).  Writes at most
 * cap - 1 characters + NUL to buf (may be NULL) and returns the full length, or a negative MI_E* code. */
int mi_debug_plan_dump(mi_plan* plan, int B, int H, int W, int side_by_side, char* buf, size_t cap);

/* Debug/test hook, host only: the staging geometry of one instantiated tile of the split-fp16 3x3 / 1x1 kernel
 * (conv_mfma_f16x3.hip: Conv16Geom) -- weight-ring slots, weight DMA pieces per wave and step, activation DMA pieces per wave
 * and chunk, LDS bytes at 384 input channels.  tests/test_dma_protocol_cpu.py replays the kernel's issue / wait protocol with
 * these numbers for every instantiated tile and checks every hand-counted `s_waitcnt vmcnt(N)`.  MI_EINVAL: not instantiated. */
int mi_debug_conv16_geometry(int ks, int stride, int tw, int mt, int nt, int wm, int wn, int cb,
                             int* ring, int* ppw, int* apw, int* lds_bytes);
/* The same for `planes` fp16 planes per operand: 2 = the split-fp16 kernel (identical to the call above), 1 = the one-product
 * kernel of MI_COMPUTE_F16 (halved image and weight slices: other ring depths and pieces per wave). */
int mi_debug_conv16_geometry_planes(int ks, int stride, int tw, int mt, int nt, int wm, int wn, int cb, int planes,
                                    int* ring, int* ppw, int* apw, int* lds_bytes);
/* Debug/test hook, host only: the number of 32-wide K steps per tile the fp16-MFMA convolution kernel walks, and the packed
 * weights hold, for (Cin, ks) with cb 16-channel blocks per chunk (0: the default of the kernel size; 2: the wide 3x3 chunks).
 * The one function kernel, packer and planner share (conv16_num_steps); the folded res_conv's steps are not included.
 * 3x3, 16-channel chunks: the pair walk, (nblk / 2) * 9 + (nblk & 1) * 5 with nblk = Cin / 16.  Negative MI_E* on bad arguments. */
int mi_debug_conv16_steps(int Cin, int ks, int cb);

/* First 16 hex digits of the sha256 over the kernel sources (csrc/ *.h, *.hip) this library was BUILT from, embedded at
 * build time: what bench.py / tools/pmc_traffic.py compare profiles against (not the working tree). */
const char* mi_source_hash(void);

/* Per-kernel timing with HIP events on the caller's stream (bench.py's roofline leg; the
 * reference's only timer for this path is time.time() around denoise(), DDIMModel.py:495-498).
 * Between mi_profile_begin and mi_profile_end every kernel launched by mi_unet_forward /
 * mi_denoise on this plan is bracketed by an event pair.  mi_profile_end synchronises the
 * recorded events and returns one entry per distinct kernel symbol: launches, summed
 * duration, and the ALGORITHMIC work of those launches (flops = 2*MACs of the contraction the
 * launch performs; bytes = the tensors it must read + write once, fp32).  Calls made while
 * profiling must not be issued concurrently from several threads. */
typedef struct mi_profile_entry {
    char   name[128];      /* kernel symbol as rocprofv3 prints it (without "void " / argument list) */
    int64_t launches;
    double total_ms;
    double flops;          /* summed over the launches */
    double bytes;
} mi_profile_entry;
int mi_profile_begin(mi_plan* plan);
int mi_profile_end(mi_plan* plan, mi_profile_entry* out, int max_entries, int* n_entries);

/* ---- THE TRAINING OBJECTIVE AS AN EVALUATION: how well a checkpoint fits a (clean, noisy) pair at a timestep ----------------------
 * The reference trains on: draw t, noise the clean image to x_t (DiffusionDenoiser.noise_images, DDIMModel.py:259-263), predict the
 * noise with one forward, and compare (DDIMModel.py:351-375; cddpmModels.py:367-374).  These calls evaluate that number -- per sample,
 * no gradients -- so that a loss-per-timestep curve of a checkpoint needs no sampler run.
 *
 * THE FORWARD NOISE (fixed).  z is the standard normal of the generator specified at mi_denoise_seeded: the same Philox4x32-10 call,
 * the same u1 and u2, the same line  z = sqrtf(-2 * logf(u1)) * cospif(2 * u2), every product rounded once.  There is NO 0.5 factor:
 * eps = z.  The counter words are
 *   c0 = element index inside the sample's [C,H,W] block, c * H*W + y * W + x   (C*H*W < 2^32)
 *   c1 = low 32 bits of sample_offset + b      (the global image index, as there)
 *   c2 = 0x80000000 | draw,  0 <= draw < 2^31  (a caller numbers the noise draws of one image 0, 1, 2, ...)
 *   c3 = 0                                      key k0, k1 = low, high word of seed
 * A sampler iteration index never has the top bit of c2 set (the slot path refuses iter_base + n_rows > 2^31 - 1; the uniform calls
 * count from 0), so no forward-noise value is a step-noise value of the same seed.
 *
 * THE NOISING (fixed).  Per sample b, on the host in fp32, in the reference's order:
 *   a_b = sqrtf(alpha_hat[t_b])        s_b = sqrtf(1.0f - alpha_hat[t_b])
 * They reach the device, with the counter words c1 and c2, as kernel arguments (records of 16 bytes a sample, at most 32 a launch): the host tables are not read after
 * the call returns.  Device, per element, fp32:  x_t = a*x + s*eps  -- two products and one sum, each rounded once, no fused
 * multiply-add: the bit pattern of the reference's expression in torch eager on a CPU.
 *
 * THE DENOISING LOSS (fixed).  Per sample b, per element, fp32, every operation rounded to nearest on its own, no fused multiply-add;
 * min / max here are torch.clamp's: a NaN stays a NaN.
 *   e = flags & MI_CLAMP_EPS ? min(max(eps_pred, -5), 5) : eps_pred
 *   d = e - eps          q = d*d
 *   p = min(max((x_t - s*e) / a, 0), 1)                 (IEEE division: the predicted clean image)
 *   Sobel cross-correlation of p and of clean, per channel, zero outside the image; with u[i][j] the 3 x 3 neighbourhood (i the row),
 *   the six non-zero taps of each kernel in row-major order, summed left to right:
 *     ex = -u00 + u02 - 2*u10 + 2*u12 - u20 + u22           (kernel [[-1,0,1],[-2,0,2],[-1,0,1]], DDIMModel.py:324)
 *     ey = -u00 - 2*u01 - u02 + u20 + 2*u21 + u22           (its transpose, DDIMModel.py:325)
 *   m(u) = sqrtf(ex*ex + ey*ey + 1e-8f)   ((ex*ex + ey*ey) first, then the constant; IEEE square root)
 *   g = |m(p) - m(clean)|
 * The sums are in double, every addition rounded on its own, no atomics, in ONE order:
 *   - a channel plane is cut into 32 x 32 patches from its top-left corner (the last ones partial); pixels outside add nothing;
 *   - inside a patch, lane j = 0 .. 255 owns column j % 32 of rows j / 32 + 8 k, k = 0, 1, 2, 3, and adds its pixels in that order
 *     starting from 0; the 256 lane sums are then folded by the tree  for off = 128, 64, .., 1: v[j] += v[j + off]  for j < off;
 *   - a sample's patch sums are added one by one, starting from 0, in (channel, patch row, patch column) order.
 *   mse_b = sum(q) / (double)(C*H*W)     edge_b = sum(g) / (double)(C*H*W)     loss_b = mse_b + edge_weight * edge_b   (double)
 * The reference's scalars are the means of these over the batch (F.mse_loss, F.l1_loss); its DDIM objective is MI_CLAMP_EPS with
 * edge_weight = 0.2, its cddpm objective no clamp and the plain MSE (edge_weight = 0; the edge term is still reported).  The host
 * shims default to those.  tests/denoising_loss_reference.py restates the three specifications in numpy.
 *
 * Arguments the calls share
 *   clean        device fp32 [B,C,H,W]
 *   t            HOST int32 [B], each in [0, noise_steps);  alpha_hat  HOST fp32 [noise_steps]
 *   eps / seeded the noise source, exactly one: eps device fp32 [B,C,H,W] (the caller's tensor), or seeded != 0 with seed,
 *                sample_offset (>= 0) and draw: the forward noise above, drawn on the device
 *   sample_index, draws   HOST int64 [B] or NULL, seeded only: per-sample counter words in the place of sample_offset + b and of draw
 *                (sample_index[b] >= 0, 0 <= draws[b] < 2^31), so that one call can hold any set of (image, draw) pairs -- a loss
 *                profile runs image b at its k-th timestep as (sample_offset + b, draw k) whatever shares the pass
 *   out          device double [B][3] = (mse, edge, loss), 8-byte aligned
 *   maps         device fp32 [3][B,C,H,W] or NULL: the per-pixel q, g and p
 *   flags        MI_CLAMP_EPS or 0;  edge_weight: any number but NaN
 * MI_EINVAL before any GPU work, the rule named in mi_last_error: a null argument; a size below 1, C > 65535, H or W > 2^30; a timestep outside
 * [0, noise_steps); a draw outside [0, 2^31); a negative sample_offset or sample_index; C*H*W >= 2^32; both a seed and eps; neither
 * a seed nor eps; sample_index or draws without a seed; a tensor that is not 4-byte aligned.  All calls allocate nothing and are asynchronous on `stream`.
 *
 * mi_noise_images (no plan needed): x_t device fp32 [B,C,H,W] <- THE NOISING of clean with eps or with the seeded draw; eps_out
 *   (device fp32 [B,C,H,W] or NULL, seeded only) receives the drawn eps.  Tensors that share their offset from a 16-byte boundary
 *   move as 16-byte words with a scalar head and tail per sample, others element by element: the same bits either way.
 * mi_loss_terms (no plan needed): THE DENOISING LOSS of a given eps_pred.  Explicit form: x_t and eps given.  Seeded form: x_t and eps
 *   NULL; z and x_t are formed again from the seed -- the same bits as the explicit form on what mi_noise_images exports.
 *   workspace: mi_loss_workspace_bytes (the patch sums), 8-byte aligned; 0 from the query on sizes the call refuses.
 * mi_denoising_loss: one enqueue, no host synchronisation: mi_noise_images into the workspace, the unchanged forward of
 *   mi_unet_forward at the per-sample t with condition cond (device fp32 [B,C,H,W]; C is the plan's in_channels), then mi_loss_terms
 *   on the same stream -- bit for bit those three calls one after another.  workspace: mi_denoising_loss_workspace_bytes = the
 *   workspace of the forward's one program (at most mi_workspace_bytes) plus the call's own region (x_t, eps_pred and the patch
 *   sums), 256-byte aligned; the status word is cleared by
 *   the call and read with mi_status as after every other call.  Further refusals: the plan's state, the workspace, a timestep
 *   outside the plan's time table, the device. */
int mi_noise_images(const float* clean, const int32_t* t, const float* alpha_hat, int noise_steps,
                    const float* eps, int seeded, uint64_t seed, int64_t sample_offset, int64_t draw,
                    const int64_t* sample_index, const int64_t* draws,
                    float* x_t, float* eps_out, int B, int C, int H, int W, void* stream);
size_t mi_loss_workspace_bytes(int B, int C, int H, int W);
int mi_loss_terms(const float* clean, const float* x_t, const float* eps, const float* eps_pred,
                  const int32_t* t, const float* alpha_hat, int noise_steps,
                  int seeded, uint64_t seed, int64_t sample_offset, int64_t draw,
                  const int64_t* sample_index, const int64_t* draws, int flags, double edge_weight,
                  double* out, float* maps, int B, int C, int H, int W,
                  void* workspace, size_t workspace_bytes, void* stream);
size_t mi_denoising_loss_workspace_bytes(mi_plan* plan, int B, int H, int W);
int mi_denoising_loss(mi_plan* plan, const float* clean, const float* cond, const int32_t* t,
                      const float* alpha_hat, int noise_steps,
                      const float* eps, int seeded, uint64_t seed, int64_t sample_offset, int64_t draw,
                      const int64_t* sample_index, const int64_t* draws, int flags, double edge_weight,
                      double* out, float* maps, int B, int H, int W,
                      void* workspace, size_t workspace_bytes, void* stream);

void mi_plan_destroy(mi_plan* plan);

/* ---- pre/post-processing either side of the sampler, on the device (no plan needed) -----------------------
 * All pointers are device pointers; `stream` is a hipStream_t (NULL = default stream); calls are asynchronous.
 *
 * mi_resize_bicubic_u8: `n` 8-bit single-channel images [n][sh][sw] -> [n][dh][dw], bit-identical to Pillow's
 *   `Image.resize((dw, dh), Image.BICUBIC)` on an 'L' image, i.e. to `transforms.Resize((dh, dw), BICUBIC)` on a
 *   PIL input (Backend/run.py:146,198; Backend/cddpm/cddpmModels.py:488,502).  `workspace` needs
 *   mi_resize_workspace_bytes(n, sw, sh, dw, dh) bytes, 256-byte aligned.
 * mi_u8_to_unit_f32: `transforms.ToTensor()` on uint8 data: x / 255 in fp32 (run.py:199).
 * mi_unit_f32_to_u8: `(clamp(x, 0, 1) * 255).astype('uint8')` (run.py:107,145): fp32 multiply, truncation.
 * mi_image_metrics: `compute_metrics` (Backend/DDIM/DDIMModel.py:290-300): per image PSNR and SSIM of
 *   clip(pred, 0, 1) against clip(target, 0, 1) with data_range = 1 (skimage defaults: 7x7 uniform window,
 *   K1 = 0.01, K2 = 0.03, sample covariance, mean over the interior); fp32 images [n][h][w], h, w >= 7;
 *   out: device double [n][2] = (psnr, ssim); workspace: mi_metrics_workspace_bytes(n, h) bytes. */
size_t mi_resize_workspace_bytes(int n, int sw, int sh, int dw, int dh);
int mi_resize_bicubic_u8(const void* src_u8, int n, int sw, int sh, void* dst_u8, int dw, int dh,
                         void* workspace, size_t workspace_bytes, void* stream);
int mi_u8_to_unit_f32(const void* src_u8, void* dst_f32, size_t count, void* stream);
int mi_unit_f32_to_u8(const void* src_f32, void* dst_u8, size_t count, void* stream);
size_t mi_metrics_workspace_bytes(int n, int h);
int mi_image_metrics(const void* target_f32, const void* pred_f32, int n, int h, int w, void* out_f64,
                     void* workspace, size_t workspace_bytes, void* stream);

/* ---- THE FLOAT RESIZE AND THE 16-BIT ELEMENT RULES: the high-bit-depth twin of the calls above ------------
 * The 8-bit calls above are the reference's contract (256 grey levels in and out).  X-ray detectors deliver 12 to 16 bits; these
 * calls carry such an image to the sampler and back without the 8-bit step (1 / 255 = 3.9e-3, twice the parity gate).
 *
 * mi_resize_bicubic_f32: `n` single-channel images [n][sh][sw] of element type `src_type` -> [n][dh][dw] of `dst_type`.
 *   The arithmetic is Pillow's 32bpc resample, `Image.fromarray(a, mode "F").resize((dw, dh), Image.BICUBIC)`, bit for bit:
 *     - separable, horizontal pass first; a pass whose size does not change is skipped;
 *     - bounds and coefficients as the 8-bit resample derives them BEFORE it rounds to fixed point: scale = in / out,
 *       support = 2 * max(1, scale), center = (xx + .5) * scale, xmin = max(0, (int)(center - support + .5)),
 *       xmax = min(in, (int)(center + support + .5)), bicubic weights (a = -.5) in double, `w /= ww` when their sum ww != 0;
 *     - an output value is `(float)ss` with `double ss = 0.0; for x in tap order: ss += (double)pixel[x] * k[x]`: sequential,
 *       every operation rounded on its own, no fused multiply-add;
 *     - float32 between the passes, nothing clipped there.
 *   Pillow's "I;16" resample is NOT reproduced (it wraps the low byte on overshoot: pixels next to a white edge come out below white); resampling
 *   the unit-float image is the 16-bit route.
 *   Element types on load and store:
 *     source MI_PIX_U8: (float)v / 255.0f (as mi_u8_to_unit_f32);  MI_PIX_U16: (float)v / 65535.0f, one correctly rounded fp32
 *     division;  MI_PIX_F32: as is.
 *     destination MI_PIX_F32: the value; with clamp01 != 0 min(max(v, 0), 1), applied to the FINAL value only.
 *     destination MI_PIX_U16: always clamped, then (uint16_t)(v * 65535.0f + 0.5f), the multiply and the add each rounded in
 *     fp32: round to nearest (there is no reference behaviour to mirror at 16 bits; u16 -> float -> u16 is the identity for all
 *     65536 values).  A NaN stores 0.
 *   The fused forms equal the separate steps (convert, resize, convert) bit for bit; with both sizes unchanged the call is the pure
 *   conversion.  `workspace`: mi_resize_f32_workspace_bytes(n, sw, sh, dw, dh) bytes, 256-byte aligned; it holds the coefficient
 *   tables (computed on the device: the call is asynchronous) and the float intermediate.
 *   MI_EINVAL before any GPU work, the rule named in mi_last_error: a null pointer; a non-positive size; an unknown element type or
 *   a destination of MI_PIX_U8 (the 8-bit destination stays mi_resize_bicubic_u8, whose arithmetic differs); n * height * width of
 *   the source, the intermediate or the destination >= 2^31; a workspace that is not 256-byte aligned or too small.
 *   mi_resize_f32_workspace_bytes returns 0 for sizes the call refuses.
 * mi_u16_to_unit_f32 / mi_unit_f32_to_u16: the two 16-bit element rules on `count` elements (null pointer: MI_EINVAL). */
#define MI_PIX_U8  0
#define MI_PIX_U16 1
#define MI_PIX_F32 2
size_t mi_resize_f32_workspace_bytes(int n, int sw, int sh, int dw, int dh);
int mi_resize_bicubic_f32(const void* src, int src_type, int n, int sw, int sh,
                          void* dst, int dst_type, int dw, int dh, int clamp01,
                          void* workspace, size_t workspace_bytes, void* stream);
int mi_u16_to_unit_f32(const uint16_t* src, float* dst, size_t count, void* stream);
int mi_unit_f32_to_u16(const float* src, uint16_t* dst, size_t count, void* stream);

/* ---- THE WINDOW: exact percentile windowing of the 16-bit path ------------------------------------------------
 * The 16-bit calls above scale by the container (v / 65535).  A 12-bit detector image in a 16-bit file then peaks at 0.0625 and the
 * network sees an almost black picture.  A window maps the occupied grey range [lo, hi] to [0, 1] before the sampler and back
 * afterwards (radiology's window/level).  Integer arithmetic or single fp32 roundings throughout: the device, the numpy restatement
 * (tests/window_reference.py) and the host recipe (image16.py) agree bit for bit.
 *
 * Histogram.  h[k], k in [0, 65535], counts the pixels of value k in one image of `count` pixels, 1 <= count <= 2^32 - 1 (uint32
 *   counts cannot overflow).  mi_histogram_u16: `n` images [n][count] (image i starts at element i * count; src 2-byte aligned) ->
 *   hist uint32 [n][65536] (16-byte aligned), zeroed by the call itself on the stream.  Counted in on-chip counters per workgroup
 *   and merged with integer atomics: the result does not depend on the order.
 * Levels from percentiles.  p_lo, p_hi doubles, finite, 0 <= p_lo < p_hi <= 100;  N = sum of h.
 *   rank r(p) = (uint64) floor(p * (double)(N - 1) / 100.0), the multiply and the divide in double, each rounded on its own;
 *   level(p) = the smallest k with h[0] + ... + h[k] > r(p)  ( = np.sort(image.ravel())[r(p)], the 0-based order statistic );
 *   lo = level(p_lo), hi = level(p_hi);  if hi == lo (a flat image, or both ranks in one bin): hi = lo + 1 when lo < 65535, else
 *   lo = hi - 1.  So 0 <= lo < hi <= 65535 always.  (A histogram of all zeros, which mi_histogram_u16 never writes, gives (0, 65535).)
 *   mi_window_levels: hist [n][65536] -> levels int32 [n][2] = (lo, hi) in DEVICE memory.  Every call below reads them there, so
 *   the recipe histogram -> levels -> load -> sampler -> store stays asynchronous on one stream.  Levels written by the caller
 *   instead (absolute grey levels) must satisfy 0 <= lo < hi <= 65535; the kernels do not check them.
 * Element rules under a window (lo, hi), d = (float)(hi - lo):
 *   load  u16:  x = min(max((float)((int)v - lo) / d, 0.0f), 1.0f) -- the integer difference is exact in fp32, then one correctly
 *               rounded fp32 division;
 *   store u16:  v = (uint16_t)(lo + (uint32_t)(min(max(x, 0), 1) * d + 0.5f)), the multiply and the add each rounded in fp32; a NaN
 *               stores lo.
 *   store(load(v)) == v for every v in [lo, hi].  THE WINDOW CLIPS: a value below lo comes back as lo, one above hi as hi.
 *   Percentiles (0, 100) give the min-max window, which clips nothing.  The window (0, 65535) is the unwindowed rule above
 *   (/ 65535, * 65535 + 0.5) bit for bit, in both directions.
 *   mi_window_u16_to_f32 / mi_window_f32_to_u16: the two rules on [n][count], image i under levels[i].
 * mi_resize_bicubic_f32_window: mi_resize_bicubic_f32 with every MI_PIX_U16 side (source, destination or both) taken under the
 *   window of its image; the other element types and the resample are unchanged, and the fused call equals window load -> float
 *   resize -> window store done separately, bit for bit.  levels == NULL: mi_resize_bicubic_f32 itself.  With levels, n <= 65535 and
 *   at least one side is MI_PIX_U16.
 * MI_EINVAL before any GPU work, the rule named in mi_last_error: a null pointer; n outside [1, 65535]; count outside [1, 2^32);
 *   percentiles that are not finite or break 0 <= p_lo < p_hi <= 100; a misaligned src or hist; the rules of mi_resize_bicubic_f32. */
int mi_histogram_u16(const uint16_t* src, int n, size_t count, uint32_t* hist, void* stream);
int mi_window_levels(const uint32_t* hist, int n, double p_lo, double p_hi, int32_t* levels, void* stream);
int mi_window_u16_to_f32(const uint16_t* src, const int32_t* levels, int n, size_t count, float* dst, void* stream);
int mi_window_f32_to_u16(const float* src, const int32_t* levels, int n, size_t count, uint16_t* dst, void* stream);
int mi_resize_bicubic_f32_window(const void* src, int src_type, int n, int sw, int sh,
                                 void* dst, int dst_type, int dw, int dh, int clamp01, const int32_t* levels,
                                 void* workspace, size_t workspace_bytes, void* stream);

/* Thread-local, never NULL. */
const char* mi_last_error(void);

/* Library version string, e.g. "midd 0.1 gfx950". */
const char* mi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* MIDD_H */
