/*
 * gmd_hip.h -- C ABI of libgmd_hip.so: the MI355X (gfx950 / CDNA4) kernels behind
 * GM-Diffusion's Stage-3 hot path (SDR+GM denoising loop, VAE decode, gain-map HDR
 * recomposition).
 *
 * The reference (Guanys-dar/GM-Diffusion) is pure Python with NO FFI / plugin / C
 * interface: the heavy arithmetic is whatever torch/cuDNN/diffusers
 * dispatch.  This ABI is therefore new; each entry point cites the reference
 * expression (file:line, relative to the reference root) whose arithmetic it
 * replaces.  The Python host side (gm-diffusion_amd/gm_diffusion) binds it with
 * ctypes; INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer unless named *_host; no allocation inside;
 *     the caller owns all buffers (workspace sizes documented per call);
 *   - every call is stream-ordered on `stream` (a hipStream_t passed as void*) and
 *     never synchronises, so calls are hipGraph-capturable;
 *   - return value: GMD_OK or an error code; gmd_last_error() returns a thread-local
 *     message for the last failing call;
 *   - activations are channels-last: [B, H*W, C] ("NHWC"); `dtype` selects the
 *     activation/weight element type (GMD_BF16 / GMD_F16 = MFMA path, GMD_F32 = parity path);
 *     biases, norm affine parameters and statistics are always float32.
 */
#ifndef GMD_HIP_H
#define GMD_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GMD_ABI_VERSION 14
#define GMD_WS_TAIL_BYTES 65536 /* see "WORKSPACE CONTRACT" at gmd_gemm_nt */

#define GMD_OK 0
#define GMD_ERR_INVALID 1     /* bad argument (shape / alignment / null) */
#define GMD_ERR_LAUNCH 2      /* hipLaunch / runtime failure */
#define GMD_ERR_UNSUPPORTED 3 /* valid request this build does not implement */

#define GMD_F32 0
#define GMD_BF16 1
#define GMD_F16 2  /* IEEE half: same kernels and layouts as GMD_BF16, float16 elements / MFMA forms */
/* float32 tensors whose contraction runs on the matrix cores as three float16 products (x = hi + lo, hi = f16(x),
 * lo = f16(x - hi); a*b ~ a_hi*b_hi + a_hi*b_lo + a_lo*b_hi with float32 accumulation: ~2^-22 relative per term, the order
 * of float32 rounding; operands must stay inside the float16 range, |x| <= 65504).  Accepted by gmd_gemm_nt, gmd_conv3x3
 * and gmd_attention only; every other entry point takes the same tensors as GMD_F32.  The reference runs its dual-UNet
 * pipeline in float32 (scripts/inference/experiments/formal_improved.py:199): this is that precision at matrix-core speed. */
#define GMD_F32S 3  /* both operands plain float32, split in the kernel */
#define GMD_F32SW 4 /* W operand pre-split by gmd_split_weights (weights: split once when a model is placed on the device) */
/* Round 4: float32 ACTIVATIONS stored pre-split -- every 32-element chunk of a row (128 bytes, the bytes of the 32 float32 values) holds
 * [hi 64 B | lo 64 B] in the order of gmd_split_weights.  As `dtype` of gmd_gemm_nt / gmd_conv3x3(_groupnorm): the A operand AND W are
 * pre-split (no conversion instruction in the main loop; results bit-identical to GMD_F32SW on the plain tensor).  As `out_dtype` of
 * gmd_gemm_nt (GEGLU and plain row epilogues of the split types) and as `dtype` of gmd_layernorm / gmd_groupnorm_colstats /
 * gmd_groupnorm_split / gmd_attention (there: Q, K, V^T plain as for GMD_F32S): float32 tensors in, the OUTPUT stored pre-split (rows
 * must be multiples of 32 elements, the buffer contiguous).  Such a tensor is
 * only ever an A (or W) operand of a contraction: nothing else reads it.  A pre-split operand (A under GMD_F32SA, W under GMD_F32SW /
 * GMD_F32SA) must start on a 128-byte boundary and have its leading dimension and batch stride in whole chunks (multiples of 32
 * elements): a column-offset view or a ragged leading dimension would be read as the wrong halves -- refused with GMD_ERR_INVALID. */
#define GMD_F32SA 5

/* epilogue activation for gmd_gemm_nt */
#define GMD_ACT_NONE 0
#define GMD_ACT_SILU 1
#define GMD_ACT_GEGLU 2 /* bf16 only: W rows interleaved in 16-row [value|gate] groups; writes [M, N/2] = h * gelu_erf(g) */
#define GMD_ACT_QUICK_GELU 3 /* x * sigmoid(1.702 x): CLIP text encoder MLP */

typedef void* gmd_stream_t;

int gmd_abi_version(void);
const char* gmd_last_error(void);

/* ------------------------------------------------------------------------------------
 * HDR tail
 * ---------------------------------------------------------------------------------- */

/* Fused Stage-3 tail, one pass over the two decoded images:
 *   sdr = clamp(sdr_dec/2+0.5, 0, 1), gm likewise      scripts/inference/generate_hdr.py:227-228,232-233
 *   u8  = (x*255) truncated                             generate_hdr.py:244-245
 *   hdr = (sdr^2.2 + eps)*(1 + gm*qmax) - eps           gm_diffusion/stage1/tone_mapping.py:68-70,
 *                                                       scripts/inference/experiments/formal_improved.py:34-45
 *   [clamp(hdr, 0, qmax+1) when flags&1]                tone_mapping.py:71
 *   hdr_file = hdr/(qmax+1)                             generate_hdr.py:27-29
 *   hdr_u16  = rint(clamp(hdr_file*65535, 0, 65535))    gm_diffusion/stage1/augmentations.py:38-41
 * Inputs: decoder outputs [B,3,H,W] (in_layout 0) or [B,H,W,3] (in_layout 1), in_dtype F32/BF16.
 * Outputs are [B,H,W,3]; any output pointer may be NULL. */
int gmd_hdr_tail(const void* sdr_dec, const void* gm_dec, int in_dtype, int in_layout,
                 int B, int H, int W, float qmax, float eps, int flags,
                 float* sdr_img, float* gm_img, uint8_t* sdr_u8, uint8_t* gm_u8,
                 float* hdr, float* hdr_file, uint16_t* hdr_u16, gmd_stream_t stream);

/* The fused tail at an OUTPUT SIZE OF ITS OWN (H, W): both operands are resampled onto it inside the kernel, so a full-size HDR is
 * written without a full-size float intermediate.  Replaces the closing lines of every Stage-3 driver of the reference:
 *   cv2.resize(sdr_image_decoded / gm_image, size, INTER_LINEAR) then apply_gm_to_sdr
 *                                  scripts/stage2/experiments/demo_training_loop.py:291-304, scheduler_tuning.py:234-320,
 *                                  accelerate_training_smoke.py:208-275, batch_size_sweep.py:266-267
 *   the gain map applied to the source picture's own pixels (original_hdr_image)    scripts/inference/generate_hdr.py:262-265
 * sdr: [B,.,hs,ws], gm_dec: [B,.,hg,wg], decoder outputs in [-1,1] in the layouts / dtypes of the entry point above (in_layout 2 =
 * [B,h*w,4], 4th channel ignored).  Per operand and output pixel: clamp(x/2+0.5, 0, 1) of each of the four taps (the scripts resize the
 * post-processed image), then the bilinear combination with half-pixel centres and edge clamp (cv2.INTER_LINEAR on float32 =
 * F.interpolate(mode="bilinear", align_corners=False)).  Per axis, output index i, n_in -> n_out, all in int32:
 *   num = max((2i+1) n_in - n_out, 0), den = 2 n_out, i0 = num / den, lambda = float(num - i0 den) / float(den), i1 = min(i0+1, n_in-1)
 *   value = (1-ly) ((1-lx) p00 + lx p01) + ly ((1-lx) p10 + lx p11)
 * An operand whose size equals (H, W) has lambda = 0 everywhere: the value is the tap itself, bit for bit.
 * flags bit 0: clamp hdr to [0, qmax+1]; bit 1: `sdr` is instead a uint8 [B,H,W,3] picture already at the output size (hs = H and
 * ws = W required), read as float(u8) / 255.0f (ToTensor).
 * Outputs: the seven of the entry point above at [B,H,W,3] plus hdr_rgbe, uint8 [B,H,W,4]: Ward's RGBE encoding of hdr_file (the
 * arithmetic of the RGBE entry point below), so a writer never reads a full-size float image back.  Any output pointer may be NULL;
 * float outputs 4-byte, hdr_u16 2-byte, hdr_rgbe 4-byte aligned.  SIZE LIMIT: B >= 1 and every one of hs, ws, hg, wg, H, W in
 * 1..16384, which keeps each integer numerator above below 2^30; anything else is GMD_ERR_INVALID before a launch. */
int gmd_hdr_tail_resized(const void* sdr, int hs, int ws, const void* gm_dec, int hg, int wg, int in_dtype, int in_layout,
                         int B, int H, int W, float qmax, float eps, int flags,
                         float* sdr_img, float* gm_img, uint8_t* sdr_u8, uint8_t* gm_u8,
                         float* hdr, float* hdr_file, uint16_t* hdr_u16, uint8_t* hdr_rgbe, gmd_stream_t stream);

/* The way in: uint8 [B,h,w,3] picture -> Resize((H, W), BILINEAR) -> ToTensor -> Normalize([0.5], [0.5]), the VAE encoder's input
 * (scripts/stage2/experiments/demo_training_loop.py:205-211, 230; scheduler_tuning.py, accelerate_training_smoke.py and
 * batch_size_sweep.py build the same transform).  The resize is the antialiased triangle filter of PIL's Image.resize(BILINEAR) /
 * F.interpolate(mode="bilinear", antialias=True), here without PIL's byte rounding between its two passes.  Per axis, n_in >= n_out:
 * tap j of output i has the integer weight numerator max(0, 2 n_in - |(2j+1) n_out - (2i+1) n_in|); n_in < n_out: the two bilinear
 * taps of the entry point above (numerators den - r and r).  Weights are normalised by their integer sum over the in-range taps; the
 * 2-D weight is the product.  Then v = resized / 255, out = (v - 0.5) / 0.5, one rounding to out_dtype (F32 / BF16 / F16).  Equal
 * sizes give ToTensor + Normalize exactly.  out_layout 0: [B,3,H,W]; 1: [B,H*W,cp] channels-last with channels 3..cp-1 zeroed (the
 * padded input of the encoder's first convolution; 3 <= cp <= 64).  SIZE LIMIT: B >= 1 and h, w, H, W in 1..16384 (numerators below
 * 2^30); anything else is GMD_ERR_INVALID before a launch. */
int gmd_prepare_sdr(const uint8_t* src, int B, int h, int w, void* out, int out_dtype, int out_layout, int cp, int H, int W,
                    gmd_stream_t stream);

/* tone_mapping.py:60-71 apply_gm_to_sdr (clamp!=0) / formal_improved.py:34-45 (clamp==0); any shape, n elements */
int gmd_apply_gm_to_sdr(const float* gm, const float* sdr, float* out, int64_t n,
                        float qmax, float eps, int clamp, gmd_stream_t stream);
/* kind 0: linear_scale_tmo tone_mapping.py:14-18; 1: hard_clip_tmo :21-26;
 * 2: mu-log (fix_mulog_tmo :29-36 with mu=500, random_tmo_cuda :50-57 with the drawn mu);
 * 3: tmo_cuda :39-47 (mu=5000, /10 pre-scale);
 * 4: decode post-process clamp(x/2+0.5, 0, 1), gm_diffusion/pipelines/stable_diffusion_gm.py:606;
 * 5: x*mu (1/scaling_factor*latents, generate_hdr.py:225); 6: x/mu (latents/scaling_factor, stable_diffusion_gm.py:1094) */
int gmd_tmo(const float* in, float* out, int64_t n, int kind, float qmax, float mu, gmd_stream_t stream);
/* tone_mapping.py:74-90 gamut_compress on [B,3,HW] planar input */
int gmd_gamut_compress(const float* in, float* out, int B, int64_t HW, gmd_stream_t stream);
/* scripts/stage1/train_vqgan_lora.py:1133-1141: apply_gm_to_sdr(clamped) -> fix_mulog_tmo -> gamut_compress, planar [B,3,HW] */
int gmd_stage1_chain(const float* gm, const float* sdr, float* out, int B, int64_t HW, float qmax, gmd_stream_t stream);
/* augmentations.py:38-41 discretize_to_uint16; out_float and/or out_codes may be NULL */
int gmd_discretize_u16(const float* in, float* out_float, uint16_t* out_codes, int64_t n, gmd_stream_t stream);
/* Radiance RGBE pixels of float RGB [npix,3] -> [npix,4] bytes (Ward's float2rgbe, the encoder behind
 * cv2.imwrite("*.hdr"), scripts/inference/generate_hdr.py:27-30); negative components are stored as 0 */
int gmd_rgbe_encode(const float* rgb, uint8_t* out, int64_t npix, gmd_stream_t stream);
/* HOST function (no device work): run-length framing of RGBE scanlines for a Radiance .hdr file, the form OpenCV's encoder
 * behind cv2.imwrite("*.hdr") (generate_hdr.py:27-30) writes by default.  rgbe: host [H][W][4] bytes from gmd_rgbe_encode;
 * out: host buffer of at least gmd_rgbe_rle_bound(H, W) bytes; *out_bytes = bytes to write after the header.  Widths < 8 or
 * > 32767 come back flat, as the format prescribes. */
int64_t gmd_rgbe_rle_bound(int H, int W);
int gmd_rgbe_rle_encode(const uint8_t* rgbe, int H, int W, uint8_t* out, int64_t capacity, int64_t* out_bytes);
/* generate_hdr.py:244-245 (x*255).astype(uint8) */
int gmd_quantize_u8(const float* in, uint8_t* out, int64_t n, gmd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * latent-side fused step
 * ---------------------------------------------------------------------------------- */

/* One pass over a [B,4,h,w] fp32 latent: classifier-free-guidance combine
 * (stable_diffusion_dual_unet.py:1063-1065), optional per-sample guidance rescale factor
 * (:1067-1069, rescale_noise_cfg :71-94; `rescale_ratio` = std_text/std_cfg per sample from
 * gmd_cfg_std_ratio), x0 prediction (:1071-1075) and the PNDM/PLMS linear-multistep update
 * (diffusers PNDMScheduler.step_plms/_get_prev_sample, called at :1077 and :1093).
 *   mode 0: eps' = eps                        (first step)
 *   mode 1: eps' = (eps + e1)/2, sample = cur_sample   (PLMS counter==1 redo step)
 *   mode 2: eps' = (3 eps - e1)/2
 *   mode 3: eps' = (23 eps - 16 e1 + 5 e2)/12
 *   mode 4: eps' = (55 eps - 59 e1 + 37 e2 - 9 e3)/24
 *   x_prev = sample_coeff*sample - (alpha_delta*eps')/denom
 * eps_in: [2B,4,h,w] (uncond half first) when do_cfg else [B,4,h,w].
 * eps_out (the guided eps, appended to the scheduler history by the host), x_prev, x0 may alias nothing.
 * Arithmetic is float32 without FMA contraction, in torch's operation order: results are
 * bit-identical to the CPU reference given identical eps. */
int gmd_latent_step(const float* eps_in, const float* x, const float* cur_sample,
                    const float* e1, const float* e2, const float* e3,
                    int B, int64_t chw, int do_cfg, float guidance_scale,
                    const float* rescale_ratio, float guidance_rescale,
                    int mode, float sample_coeff, float alpha_delta, float denom,
                    float sqrt_alpha, float sqrt_one_minus_alpha,
                    float* eps_out, float* x_prev, float* x0, gmd_stream_t stream);

/* DPM-Solver++ multistep (dpmsolver++ / midpoint / epsilon, orders 1-2) -- the scheduler the reference swaps in for the
 * dual-UNet runs (scripts/inference/experiments/formal_improved.py:195) -- fused with the same CFG combine / rescale and
 * pipeline x0 as gmd_latent_step:
 *   m0 = (x - sigma_s0*eps)/alpha_s0;  x_prev = c_x*x - c_m*m0 [ - c_h*(inv_r0*(m0 - m1)) when order == 2 ]
 * c_x = sigma_t/sigma_s0, c_m = alpha_t*(exp(-h)-1), c_h = 0.5*c_m, inv_r0 = 1/r0: float32 scalars computed by the host
 * exactly as diffusers computes its 0-dim tensors.  m0_out is the x0 prediction the host keeps for the next step. */
int gmd_dpm_step(const float* eps_in, const float* x, const float* m1, int B, int64_t chw,
                 int do_cfg, float guidance_scale, const float* rescale_ratio, float guidance_rescale,
                 int order, float sigma_s0, float alpha_s0, float c_x, float c_m, float c_h, float inv_r0,
                 float sqrt_alpha, float sqrt_one_minus_alpha,
                 float* m0_out, float* x_prev, float* x0, gmd_stream_t stream);

/* SDE-DPM-Solver++ multistep ("DPM++ 2M SDE": algorithm_type "sde-dpmsolver++", midpoint / heun, epsilon, orders 1-2) -- the
 * stochastic sampling the reference's dual-UNet runs ask for with `eta=0.7  # Controls stochasticity`
 * (scripts/inference/experiments/formal_improved.py:195, 267), which DPM-Solver has no `eta` for.  Added within ABI v14 (purely
 * additive: no existing signature changed).  Fused with the same CFG combine / rescale and pipeline x0 as gmd_latent_step, in
 * the float32 operation order of diffusers' dpm_solver_first_order_update / multistep_dpm_solver_second_order_update:
 *   m0 = (x - sigma_s0*eps)/alpha_s0;  x_prev = c_x*x + c_m*m0 [ + c_h*(inv_r0*(m0 - m1)) when order == 2 ] + c_n*noise
 * c_x = sigma_t/sigma_s0*exp(-h), c_m = alpha_t*(1 - exp(-2h)), c_n = sigma_t*sqrt(1 - exp(-2h)), inv_r0 = 1/r0 and
 * c_h = 0.5*c_m (midpoint) or alpha_t*((1 - exp(-2h))/(-2h) + 1) (heun): float32 scalars computed by the host exactly as
 * diffusers computes its 0-dim tensors.  The noise is required and added at EVERY step, also with c_n == 0 (the last step of
 * a final_sigmas_type "zero" schedule); it is drawn by the host scheduler from the caller's generator, in the reference's
 * order (SDR first, GM second).  m0_out is the x0 prediction the host keeps for the next step; x0 may be NULL.  c_n must be
 * >= 0 (a NaN is refused).  The deterministic heun solver type needs no entry point of its own: it is gmd_dpm_step with
 * c_h = -alpha_t*((exp(-h) - 1)/h + 1), since a - (-k)*d and a + k*d are the same float32 value. */
int gmd_dpm_sde_step(const float* eps_in, const float* x, const float* m1, const float* noise, int B, int64_t chw,
                     int do_cfg, float guidance_scale, const float* rescale_ratio, float guidance_rescale,
                     int order, float sigma_s0, float alpha_s0, float c_x, float c_m, float c_h, float inv_r0, float c_n,
                     float sqrt_alpha, float sqrt_one_minus_alpha,
                     float* m0_out, float* x_prev, float* x0, gmd_stream_t stream);

/* DDPM ancestral step -- the scheduler the reference's Stage-3 CLI constructs (scripts/inference/generate_hdr.py:162,
 * used by the pipeline call at :212-218) -- fused with the same CFG combine / rescale and pipeline x0 as gmd_latent_step,
 * in the float32 operation order of diffusers' DDPMScheduler.step:
 *   p0 = (x - sched_sqrt_one_minus_alpha*eps)/sched_sqrt_alpha [clamp +-clip_range];  x_prev = x0_coeff*p0 + xt_coeff*x
 *   [ + noise_scale*noise when noise != NULL (t > 0) ].
 * `noise` is drawn by the host scheduler from the caller's generator, so a generator shared by the two schedulers of the
 * dual pipeline is consumed SDR first, GM second (stable_diffusion_dual_unet.py:1015, 1077, 1093). */
int gmd_ddpm_step(const float* eps_in, const float* x, const float* noise, int B, int64_t chw,
                  int do_cfg, float guidance_scale, const float* rescale_ratio, float guidance_rescale,
                  float sched_sqrt_alpha, float sched_sqrt_one_minus_alpha, int clip_sample, float clip_range,
                  float x0_coeff, float xt_coeff, float noise_scale, float sqrt_alpha, float sqrt_one_minus_alpha,
                  float* x_prev, float* x0, gmd_stream_t stream);

/* DDIM step -- the scheduler the pipelines' docstrings name first (stable_diffusion_gm.py:188, stable_diffusion_dual_unet.py:188)
 * and the only one that uses their `eta` argument (:612, :843) -- fused with the same CFG combine / rescale and pipeline x0 as
 * gmd_latent_step, in the float32 operation order of diffusers' DDIMScheduler.step (epsilon prediction):
 *   p0 = (x - sched_sqrt_one_minus_alpha*eps)/sched_sqrt_alpha [clamp +-clip_range]          pred_original_sample
 *   pe = use_clipped ? (x - sched_sqrt_alpha*p0)/sched_sqrt_one_minus_alpha : eps             pred_epsilon
 *   x_prev = sqrt_alpha_prev*p0 + dir_coeff*pe [ + std_dev*noise when noise != NULL (eta > 0) ]
 * sqrt_alpha_prev = a_prev ** 0.5, std_dev = eta * variance ** 0.5, dir_coeff = (1 - a_prev - std_dev^2) ** 0.5: float32
 * scalars computed by the host exactly as diffusers computes its 0-dim tensors.  The noise is added whenever it is given,
 * also with std_dev == 0 (diffusers adds it iff eta > 0, at every step); it is drawn by the host scheduler from the caller's
 * generator, in the reference's order (SDR first, GM second).  x0 (the pipeline's, never clipped) and pred_x0 (the clipped p0,
 * diffusers' pred_original_sample) may be NULL.  dir_coeff and std_dev must be >= 0 (a NaN is refused). */
int gmd_ddim_step(const float* eps_in, const float* x, const float* noise, int B, int64_t chw,
                  int do_cfg, float guidance_scale, const float* rescale_ratio, float guidance_rescale,
                  float sched_sqrt_alpha, float sched_sqrt_one_minus_alpha, int clip_sample, float clip_range,
                  int use_clipped, float sqrt_alpha_prev, float dir_coeff, float std_dev,
                  float sqrt_alpha, float sqrt_one_minus_alpha,
                  float* x_prev, float* x0, float* pred_x0, gmd_stream_t stream);

/* Latent-consistency (LCM) step -- diffusers' LCMScheduler.step (epsilon prediction), the few-step sampler of a guidance-embedded
 * UNet (time_cond_proj_dim; stable_diffusion_gm.py:1024-1030, stable_diffusion_dual_unet.py:1024-1030) -- fused with the same CFG
 * combine / rescale and pipeline x0 as gmd_latent_step, in the float32 operation order of its torch expressions.  Added within
 * ABI v14 (purely additive: no existing signature changed).
 *   p0 = (x - sched_sqrt_one_minus_alpha*eps)/sched_sqrt_alpha [clamp +-clip_range]          predicted_original_sample
 *   denoised = c_out*p0 + c_skip*x                                                           boundary-condition scalings
 *   x_prev = noise != NULL ? sqrt_alpha_prev*denoised + sqrt_beta_prev*noise : denoised      noise == NULL at the last step
 * c_skip = sigma_data^2/(s^2 + sigma_data^2), c_out = s/(s^2 + sigma_data^2)^0.5 with s = t*timestep_scaling, sigma_data = 0.5,
 * sqrt_alpha_prev = a_prev ** 0.5, sqrt_beta_prev = (1 - a_prev) ** 0.5: float32 scalars computed by the host.  The noise is drawn
 * by the host scheduler from the caller's generator, in the reference's order (SDR first, GM second).  x0 (the pipeline's, never
 * clipped) and denoised may be NULL; nothing else is stored.  Refused before any launch: a non-finite coefficient (a NaN is
 * refused), a zero denominator, a clip_range <= 0 with clip_sample. */
int gmd_lcm_step(const float* eps_in, const float* x, const float* noise, int B, int64_t chw,
                 int do_cfg, float guidance_scale, const float* rescale_ratio, float guidance_rescale,
                 float sched_sqrt_alpha, float sched_sqrt_one_minus_alpha, int clip_sample, float clip_range,
                 float c_skip, float c_out, float sqrt_alpha_prev, float sqrt_beta_prev,
                 float sqrt_alpha, float sqrt_one_minus_alpha,
                 float* x_prev, float* x0, float* denoised, gmd_stream_t stream);

/* Euler / Euler-ancestral step (diffusers' EulerDiscreteScheduler and EulerAncestralDiscreteScheduler, epsilon prediction, no
 * churn) fused with the same CFG combine / rescale as gmd_latent_step, in the float32 operation order of their torch expressions:
 *   p0 = x - sigma_hat*eps;  d = (x - p0)/sigma_hat;  x_prev = x + d*dt [ + noise*sigma_up when noise != NULL (ancestral) ]
 * dt = sigma_next - sigma_hat (Euler) or sigma_down - sigma (ancestral), float32 scalars computed by the host exactly as
 * diffusers computes its 0-dim tensors.  The noise is added whenever it is given, also with sigma_up == 0 (the ancestral
 * scheduler adds it at every step); it is drawn by the host scheduler from the caller's generator, SDR first, GM second.
 * pred_x0 (p0: diffusers' pred_original_sample and, in sigma space, the pipeline's x0 that the dual pipeline hands to the GM
 * UNet) may be NULL.  Refused before any launch: !(sigma_hat > 0), !(sigma_up >= 0) (a NaN is refused), a non-finite dt. */
int gmd_euler_step(const float* eps_in, const float* x, const float* noise, int B, int64_t chw,
                   int do_cfg, float guidance_scale, const float* rescale_ratio, float guidance_rescale,
                   float sigma_hat, float dt, float sigma_up, float* x_prev, float* pred_x0, gmd_stream_t stream);

/* Linear multistep step (diffusers' LMSDiscreteScheduler, epsilon prediction, orders 1-4) fused with the same CFG combine /
 * rescale as gmd_latent_step, in the float32 operation order of its torch expressions:
 *   p0 = x - sigma*eps;  d = (x - p0)/sigma;  acc = 0.0f + c0*d [+ c1*d1 [+ c2*d2 [+ c3*d3]]];  x_prev = x + acc
 * d1, d2, d3 are the derivatives of the previous 1, 2, 3 steps (d_out of those launches); d(order) and beyond are never
 * read, nor are their coefficients.  The sum starts from 0.0f because Python's sum() starts from int 0: 0 + (-0.0) is +0.0.
 * c0..c3 are the integrals over [sigma, sigma_next] of the Lagrange basis polynomials on the last `order` sigmas, computed by
 * the host in float64 and rounded to float32 by this argument.  d_out (the derivative, which the host keeps as history) and
 * x_prev are always written; pred_x0 (p0: diffusers' pred_original_sample and the pipeline's x0) may be NULL.  d_out must
 * not alias an input.  Refused before any launch: order outside 1..4, !(sigma > 0) (a NaN is refused), a non-finite
 * coefficient among c0..c(order-1), a null d1..d(order-1). */
int gmd_lms_step(const float* eps_in, const float* x, const float* d1, const float* d2, const float* d3, int B, int64_t chw,
                 int do_cfg, float guidance_scale, const float* rescale_ratio, float guidance_rescale,
                 int order, float sigma, float c0, float c1, float c2, float c3,
                 float* d_out, float* x_prev, float* pred_x0, gmd_stream_t stream);

/* UniPC predictor-corrector step (diffusers' UniPCMultistepScheduler: predict_x0, epsilon prediction, bh1 / bh2, orders 1-3) fused
 * with the same CFG combine / rescale as gmd_latent_step, in the float32 operation order of the scheduler's torch expressions.
 * h1, h2, h3: the x0 predictions of the previous 1, 2, 3 steps (m0_out of those launches); last_sample: x_corr of the previous launch.
 *   m0 = (x - sigma_s*eps)/alpha_s                                   from x as it comes in, before the correction
 *   corrector, order corr_order = p in 0..3 (0: off, x_corr = x):
 *     acc = c_rho1*((h2 - h1)/c_r1) [+ c_rho2*((h3 - h1)/c_r2)] + c_rho<p>*(m0 - h1)       (p = 1: c_rho1*(m0 - h1) alone)
 *     x_corr = c_x*last_sample - c_m*h1 - c_b*acc
 *   predictor, order pred_order = q in 1..3:
 *     x_prev = p_x*x_corr - p_m*m0 [- p_b*(p_rho1*((h1 - m0)/p_r1) [+ p_rho2*((h2 - m0)/p_r2)])]   (q = 1: no p_b term at all)
 * c_x / p_x = sigma_t/sigma_s, c_m / p_m = alpha_t*phi_1, c_b / p_b = alpha_t*B_h of the corrected / predicted interval.  The kernel
 * divides by r_k.  m0_out (the host's history), x_corr (the host's next last_sample: a copy of x when the corrector is off) and x_prev
 * are always written; x0 (the pipeline's (x - sqrt_one_minus_alpha*eps)/sqrt_alpha) may be NULL.  No output may alias an input.
 * A pointer or scalar beyond the orders in use is neither read nor checked.  Refused before any launch: an order out of range, a
 * non-finite scalar or a zero divisor among those in use, a null pointer among those in use. */
int gmd_unipc_step(const float* eps_in, const float* x, const float* last_sample, const float* h1, const float* h2, const float* h3,
                   int B, int64_t chw, int do_cfg, float guidance_scale, const float* rescale_ratio, float guidance_rescale,
                   int corr_order, int pred_order, float sigma_s, float alpha_s,
                   float c_x, float c_m, float c_b, float c_rho1, float c_rho2, float c_rho3, float c_r1, float c_r2,
                   float p_x, float p_m, float p_b, float p_rho1, float p_rho2, float p_r1, float p_r2,
                   float sqrt_alpha, float sqrt_one_minus_alpha,
                   float* m0_out, float* x_corr, float* x_prev, float* x0, gmd_stream_t stream);

/* per-sample unbiased std of the text eps and of the guided eps -> ratio[b] = std_text/std_cfg
 * (rescale_noise_cfg, stable_diffusion_dual_unet.py:88-91) */
int gmd_cfg_std_ratio(const float* eps_in, int B, int64_t chw, float guidance_scale,
                      float* ratio, gmd_stream_t stream);

/* img2img start and inpaint blend of one step over [B, C, hw] float32 latents, one launch for what torch writes as
 *   keep   = scheduler.add_noise(z0, noise, t_next)  ==  ca * z0 + cb * noise     (noise == NULL, the last step: keep = z0)
 *   x_prev = (1 - m) * keep + m * x_prev                                          (mask == NULL: x_prev = keep, x_prev is not read)
 *   x0     = (1 - m) * z0 + m * x0                                                (x0 may be NULL)
 * in that float32 operation order, no FMA contraction; m = mask[(mask_rows == 1 ? 0 : b) * hw + p], broadcast over the channels,
 * any float value (1 = repaint, 0 = keep; no shortcut at 0 or 1, so 0 * inf is NaN as in torch).  x_prev and x0 are updated in
 * place.  (ca, cb) come from the scheduler's add_noise_coefs.  B * C * hw == 0 is a no-op.  Refused before any launch: a null z0,
 * both outputs null, x0 without a mask, mask_rows neither 1 nor B. */
int gmd_inpaint_blend(float* x_prev, float* x0, const float* mask, const float* z0, const float* noise, int B, int C, int64_t hw,
                      int mask_rows, float ca, float cb, gmd_stream_t stream);

/* 8-channel concat + CFG duplicate + NCHW->NHWC + cast + zero channel padding in one pass
 * (stable_diffusion_gm.py:1045-1047 cat([sdr_latent, latents],1) then cat([.]*2);
 *  stable_diffusion_dual_unet.py:1045, 1080).  src0 [B,C0,HW] f32, src1 [B,C1,HW] f32 or NULL;
 * out [dup*B, HW, CP] of out_dtype with channels >= C0+C1 zeroed. */
int gmd_pack_unet_input(const float* src0, int C0, const float* src1, int C1, int B, int64_t HW,
                        int dup, void* out, int CP, int out_dtype, gmd_stream_t stream);
/* gmd_pack_unet_input with each source divided by its own float32 divisor before the one rounding to out_dtype: the
 * scale_model_input of a sigma-space scheduler (sample / ((sigma**2 + 1) ** 0.5)) folded into the pack.  val = s / div is a
 * float32 division (no reciprocal multiply), so div == 1.0f reproduces gmd_pack_unet_input bit for bit; padding channels stay
 * zero.  div0 and (when C1 > 0) div1 must be > 0 (a NaN is refused). */
int gmd_pack_unet_input_scaled(const float* src0, int C0, float div0, const float* src1, int C1, float div1,
                               int B, int64_t HW, int dup, void* out, int CP, int out_dtype, gmd_stream_t stream);
/* [B,HW,ld] (first C channels) of in_dtype -> [B,C,HW] float32 */
int gmd_unpack_nchw(const void* in, int in_dtype, int64_t ld, int B, int C, int64_t HW,
                    float* out, gmd_stream_t stream);

/* ------------------------------------------------------------------------------------
 * UNet / VAE building blocks (arithmetic lives in the un-vendored
 * `diffusers` dependency: UNet2DConditionModel / AutoencoderKL called at
 * stable_diffusion_gm.py:1051,1094 and stable_diffusion_dual_unet.py:1052,1083)
 * ---------------------------------------------------------------------------------- */

/* DEBUG ONLY -- kernel-tuning hook of tools/ (bench_gemm.py, check_ring.py, bench_graph_ops.py); never called by the product
 * path and refused (GMD_ERR_UNSUPPORTED) unless the process has GMD_TUNING=1 in its environment.  Pins the tile (bm x bn), the
 * operand pipeline (pf: 9 = LDS-DMA, 1/2 = register staged, 1xx = ring variants) and the split-K factor of every later 16-bit
 * gmd_gemm_nt / gmd_conv3x3 launch of this process; 0 keeps the heuristic for that field, (0,0,0,0) restores it (always
 * allowed).  GMD_GEMM_FORCE="bm,bn,pf,ksplit" seeds the same override when the library is loaded, under the same GMD_TUNING
 * gate.  A forced plan whose kernel lacks the epilogue a launch asks for (fused GEGLU, column statistics) is refused at the
 * launch, never run. */
int gmd_gemm_plan_override(int bm, int bn, int pf, int ksplit);

/* Plan family of the CALLING THREAD's later 16-bit gmd_gemm_nt / gmd_conv3x3 / gmd_gemm_qkv_vt launches (and of the plan queries
 * gmd_gemm_colstats_plan / gmd_gemm_plan_info / gmd_gemm_qkv_vt_ok, which must agree with them): 0 (the default) = the plan that is
 * fastest when the launch has the chip to itself; 1 = the co-running family (256-row tiles, filled up with K slices: fewest L2 -> LDS
 * bytes per product) for launches that share the chip with a second stream's kernels -- what the dual-UNet pipeline selects around
 * its two overlapped forwards (stable_diffusion_dual_unet.py:1040-1093: the two UNet calls of one loop iteration).  Results of the
 * two families agree to float32 summation order (K slices).  Returns the previous family; any other argument only queries.  Thread-
 * local, so concurrent host threads do not see each other's choice.  GMD_PP=b / GMD_PP=1 in the environment pin 1 / 0 process-wide. */
int gmd_gemm_plan_family(int family);

/* Split-K launches of the 16-bit gmd_gemm_nt / gmd_conv3x3 with up to `max_slices` K slices reduce INSIDE the kernel (the last
 * slice of a tile adds the others' accumulator fragments in slice order and runs the fused epilogue: no partial-sum slabs, no
 * reduction launch); more slices, and launches whose consumer reads the slabs itself (gmd_conv3x3_groupnorm), keep the slab path.
 * Both paths add the same partial sums in the same order: results are bit-identical.  Default 4 (GMD_SPLITK_FIXUP=<n> in the
 * environment seeds it; 0 = slab path everywhere).  Returns the previous value; a negative argument only queries.  Process-wide:
 * change it only while no launch is in flight (tests, A/B measurements). */
int gmd_splitk_fixup_max(int max_slices);

/* C[b] = act(alpha * A[b] @ W[b]^T + bias + rowbias + residual).
 * A: [M,K] ld lda; W: [N,K] ld ldw (both K-contiguous); C: [M,N] ld ldc, out_dtype F32 or `dtype`.
 * bias: float32 [N] or NULL.  rowbias: float32 [ceil(M/rows_per_group), ldrb] (ldrb >= N; 0 means N) or NULL, added to rows
 * of group m/rows_per_group (ResnetBlock2D time-embedding add).  residual: `dtype` [M,N] ld ldr or NULL.
 * Requirements: K % 64 == 0 (BF16 / F16), K % 32 == 0 (F32S / F32SW), K % 4 == 0 (F32); lda, ldw multiples of 8 (16-bit) /
 * 4 (float32) elements (ldw of a pre-split W counts k's, as for the plain matrix);
 * base pointers 16-byte aligned.  nn.Linear / conv1x1 / attention score products.
 * workspace (optional, float32 scratch of workspace_bytes): lets launches that cannot fill the chip split K
 * (deterministic: partial sums are added in slice order, no floating-point atomics); with NULL / too small a workspace K is not split.
 * WORKSPACE CONTRACT (ABI v11; every entry point that takes a workspace): the last GMD_WS_TAIL_BYTES of the buffer are reserved for
 * the library's split-K arrival counters -- they must be ZERO when a buffer is first handed to the library (memset it once after
 * allocating it) and every launch leaves them zero; only workspace_bytes - GMD_WS_TAIL_BYTES are used for partial sums, and the plan
 * queries (gmd_gemm_colstats_plan, gmd_gemm_plan_info, gmd_gemm_qkv_vt_ok, gmd_gemm_out_split_ok, gmd_conv3x3_gn_fusable) take the
 * same workspace_bytes the launch will get.  One workspace serves ONE stream (or one captured graph) at a time: launches that may
 * run concurrently need workspaces of their own.
 * SCRATCH EXTENTS.  With usable = workspace_bytes - GMD_WS_TAIL_BYTES, a launch of ks > 1 K slices writes, from the start of the buffer,
 *   slab extent     = ks * M * N * 4 bytes (one float32 [M, N] slab per slice, summed by a reduction launch or by the GroupNorm of
 *                     gmd_conv3x3_groupnorm), or
 *   fragment extent = (ks - 1) * tiles * bm * bn * 4 bytes, tiles = ceil(M / bm) * ceil(N / bn) (the in-kernel reduction of
 *                     gmd_splitk_fixup_max: whole accumulator tiles of the slices 0 .. ks-2, ragged tiles included),
 * and nothing else: no byte at or beyond `usable` other than the counters, which end at zero, and no byte at or beyond workspace_bytes.
 * K is split into ks slices only if the slab extent of ks fits `usable`: where it does not, the planner takes fewer slices or none (a
 * slice count forced with gmd_gemm_plan_override: none, ks = 1); the in-kernel reduction is taken only if, in addition, the fragment
 * extent fits `usable` and tiles <= GMD_WS_TAIL_BYTES / 4 (otherwise: slabs).  Both give the same bits.
 * DISPATCH-ORDER ASSUMPTION of the in-kernel reduction: the last slice of a tile waits (bounded) for the other slices' workgroups, so
 * those must already hold a CU: the library relies on the hardware dispatching workgroups in increasing linear id (x fastest, the K
 * slice z slowest), round-robin over the XCDs.  There is no release / acquire pair between the slices; the hand-off rests on the
 * cache-coherence bits of the fragment stores and loads and an agent-scope counter.  GMD_SPLITK_FIXUP=0 in the environment (or
 * gmd_splitk_fixup_max(0)) is the escape hatch: every split launch then takes the slab path. */
int gmd_gemm_nt(const void* A, const void* W, void* C, int dtype, int out_dtype,
                int M, int N, int K, int64_t lda, int64_t ldw, int64_t ldc,
                int batch, int64_t strideA, int64_t strideW, int64_t strideC,
                const float* bias, const float* rowbias, int rows_per_group, int64_t ldrb,
                const void* residual, int64_t ldr, int64_t strideR,
                float alpha, int act, float* colstats, int colstats_bucket,
                void* workspace, int64_t workspace_bytes, gmd_stream_t stream);

/* Pre-split layout of a float32 weight matrix W [N,K] (row stride ldw, K % 32 == 0) for GMD_F32SW: `out` holds N*K*4 bytes,
 * per row n and block of 32 k's 64 bytes of float16 hi followed by 64 bytes of float16 lo, each as four 16-byte chunks
 * q = 0..3 holding k = {4q..4q+3, 16+4q..16+4q+3} of the block (the k's one MFMA lane group consumes).  For a convolution
 * weight [Cout, 9*Cin] (k = tap*Cin + c, Cin % 32 == 0) the same call applies with K = 9*Cin. */
int gmd_split_weights(const float* W, void* out, int64_t N, int64_t K, int64_t ldw, gmd_stream_t stream);

/* Column statistics for a following GroupNorm (diffusers GroupNorm over a ResnetBlock2D / Transformer2DModel input: the
 * statistics pass is folded into the epilogue of the launch that produces the tensor).  With `colstats` non-NULL,
 * gmd_gemm_nt / gmd_conv3x3 also write float32 colstats[M/64][N/colstats_bucket][2] = {sum, sum of squares} of the STORED
 * (rounded) outputs over each block of 64 rows and each bucket of `colstats_bucket` adjacent columns, in a fixed order.
 * Only launches that run the full-tile row epilogue of the 128-row ring kernels can do this (16-bit types, batch 1, no
 * split-K, M % 128 == 0, N a multiple of the 160- or 128-column tile, bucket dividing half a tile): this returns 1 when a
 * launch of these dimensions will, 0 otherwise (asking for colstats then fails with GMD_ERR_UNSUPPORTED).  For a
 * convolution pass M = B*Hout*Wout, N = Cout, K = 9*Cin. */
int gmd_gemm_colstats_plan(int dtype, int M, int N, int K, int batch, int64_t workspace_bytes, int bucket);

/* Which kernel a 16-bit gmd_gemm_nt / gmd_conv3x3 launch of these dimensions takes (for a convolution M = B*Hout*Wout, N = Cout,
 * K = 9*Cin; `geglu` = 1 for GMD_ACT_GEGLU launches): out4 = {tile rows, tile columns, kernel code, K slices}.  Kernel codes:
 * 0 = the LDS-DMA ring kernels (two 4-wave workgroups per CU; 64x64 tiles for under-filled launches), 283 = the ping-pong kernel
 * (one workgroup of 8 consumer + 4 loader waves on a 256-row tile, round 4), 244 = the loader / consumer kernel (4 consumer + 4
 * loader waves on a 128- or 64-row tile, for launches with about one tile per CU, round 4).  Pure host function: tests and measurement tools use
 * it to know what they exercise; nothing in the product path calls it.  Returns GMD_ERR_INVALID for other element types. */
int gmd_gemm_plan_info(int dtype, int M, int N, int K, int batch, int64_t workspace_bytes, int geglu, int* out4);

/* Fused Q|K|V projection of a self-attention (round 4, 16-bit types): C[M, vt_col0] (row stride ldc) = alpha * A[M,K] W[0:vt_col0, K]^T as
 * gmd_gemm_nt writes it, and the remaining N - vt_col0 columns (the V projection) TRANSPOSED, the way gmd_attention reads V:
 * Vt[sample][column - vt_col0][token] with row stride vt_ld, `vt_tokens` consecutive rows of A per sample.  One launch instead of the
 * projection plus a batched transposed GEMM per attention.  gmd_gemm_qkv_vt_ok: 1 when the launch's plan can do it (full tiles, the V
 * columns on a tile boundary, vt_tokens a multiple of 64); otherwise use gmd_gemm_nt twice.
 * reference: Attention.to_q / to_k / to_v of diffusers as called at gm_diffusion/pipelines/stable_diffusion_dual_unet.py:1052 */
int gmd_gemm_qkv_vt_ok(int dtype, int M, int N, int K, int vt_col0, int vt_tokens, int64_t workspace_bytes);
int gmd_gemm_qkv_vt(const void* A, const void* W, void* C, void* Vt, int dtype, int M, int N, int K, int64_t ldc, int vt_col0, int vt_tokens,
                    int64_t vt_ld, float alpha, void* workspace, int64_t workspace_bytes, gmd_stream_t stream);

/* 1 when a float32-split gmd_gemm_nt launch of these dimensions (batch 1) can take out_dtype = GMD_F32SA, i.e. store its [M, N] (GEGLU:
 * [M, N/2]) result pre-split for the contraction that follows: an unsplit launch of full 128-row tiles through the row epilogues. */
int gmd_gemm_out_split_ok(int M, int N, int K, int geglu, int64_t workspace_bytes);

/* K slices a float32 matrix-core gmd_gemm_nt launch (GMD_F32S / GMD_F32SW / GMD_F32SA, batch 1, no GEGLU) of these dimensions takes with
 * this workspace: > 1 = float32 slabs (the slab extent of the WORKSPACE CONTRACT) summed by a reduction launch.  0 for a shape the
 * path does not take (K % 32 != 0).  Pure host function: tests use it to know what they exercise. */
int gmd_split_plan_ksplit(int M, int N, int K, int64_t workspace_bytes);

/* Which kernel a float32 matrix-core gmd_gemm_nt / gmd_gemm_qkv_vt / gmd_conv3x3 launch of these dimensions takes (`dtype`: GMD_F32S,
 * GMD_F32SW or GMD_F32SA; for a convolution M = B*Hout*Wout, N = Cout, K = 9*Cin; `geglu` = 1 for GMD_ACT_GEGLU launches): out4 =
 * {tile rows, tile columns, kernel code, K slices}, the twin of gmd_gemm_plan_info.  Kernel codes: 0 = the ring kernel, every wave
 * splitting its own fragments (128x160, 128x128 or 64x64 tiles); 244 = the loader / converter kernel (128-row tiles, pre-split weights
 * with a plain activation only, i.e. GMD_F32SW; off unless GMD_SPLIT_LC=1 or a plan override selects it).  K slices > 1: float32 slabs
 * summed by a reduction launch (or by the fused GroupNorm).  A batched launch has no workspace and never slices.  Pure host
 * function: tests use it to know what they exercise.  Returns GMD_ERR_INVALID for other element types or K % 32 != 0. */
int gmd_split_plan_info(int dtype, int M, int N, int K, int batch, int64_t workspace_bytes, int geglu, int* out4);

/* Debug facility like gmd_gemm_plan_override (refused unless the process has GMD_TUNING=1): how stride-1 gmd_conv3x3 launches on
 * 256-row ping-pong tiles fetch their activations -- 2 (the default) = the tile's input patch resident in LDS, continuous consumers;
 * 1 = patch resident, ping-pong consumers; 0 = the per-tap implicit GEMM.  Results agree to rounding (the K order differs).  Seeded
 * from GMD_CONV_PATCH when the library is loaded. */
int gmd_conv_patch_override(int mode);

/* Measurement only: a one-thread kernel that writes the device's constant-rate 100 MHz counter into base[*row * stride + k] (device
 * memory; `row` may be NULL = row 0) at its place in `stream` -- also inside a captured HIP graph, where `row` (a device scalar the host
 * rewrites between replays) lets every replay fill its own row.  tools/timeline.py places such stamps at the block boundaries of both
 * UNet forwards to record the concurrent timeline of the two-stream pipeline. */
int gmd_stamp(uint64_t* base, const int* row, int stride, int k, gmd_stream_t stream);

/* GEGLU feed-forward of a BasicTransformerBlock in ONE launch (diffusers FeedForward: ff.net.0 = GEGLU(C -> 4C), ff.net.2 =
 * Linear(4C -> C); the reference reaches it through UNet2DConditionModel at stable_diffusion_dual_unet.py:1052, 1083):
 *   Y = (value * gelu_erf(gate)) @ W2^T + b2 + residual,  [value | gate] = X @ W1i^T + b1i
 * X, residual, Y: [M, C] of `dtype` (16-bit); W1i [8C, C] / b1i [8C]: ff.net.0.proj with value / gate rows interleaved in
 * 16-row groups (the layout of GMD_ACT_GEGLU); W2 [C, 4C], b2 [C].  The [M, 4C] GEGLU tensor stays on chip.  Instantiated
 * where a 128-row block's output fits the register file: gmd_ff_geglu_fused_supported() says whether (dtype, M, C) is
 * (C == 320, M % 128 == 0); elsewhere use gmd_gemm_nt(GMD_ACT_GEGLU) + gmd_gemm_nt. */
int gmd_ff_geglu_fused_supported(int dtype, int64_t M, int C);
int gmd_ff_geglu_fused(const void* X, const void* W1i, const float* b1i, const void* W2, const float* b2, const void* residual,
                       void* Y, int dtype, int64_t M, int C, gmd_stream_t stream);

/* 3x3 convolution, padding 1, as an implicit GEMM over channels-last data.
 * X: [B,Hin,Win,Cin]; Wt: [Cout, 9*Cin] with k = (ky*3+kx)*Cin + c; Y: [B,Hout,Wout,Cout].
 * stride 1 or 2 (Downsample2D: Hout = (Hin+2-3)/2+1); upsample=1 fuses nearest-2x
 * (Upsample2D: conv over the virtual 2Hin x 2Win image).  pad_mode 0: symmetric padding 1;
 * pad_mode 1: pad (0,1,0,1) then stride 2 (VAE encoder Downsample2D(padding=0)).
 * upsample = GMD_UPSAMPLE_TO(Hout, Wout) (ABI v12) fuses nearest upsampling to a GIVEN size, each side 2*in - 1 or 2*in: diffusers'
 * Upsample2D.forward(hidden_states, output_size) = conv(F.interpolate(hidden_states, size=output_size, mode="nearest")), which
 * UNet2DConditionModel takes (upsample_size = down_block_res_samples[-1].shape[2:]) when a latent side is not a multiple of
 * 2 ** (levels - 1): a stride-2 level maps H -> ceil(H / 2), so the way back up meets a skip of 2 Hin - 1 or 2 Hin rows.  For
 * exactly those sizes torch's nearest map is src = dst >> 1, the 2x map with the virtual image cut at Hout x Wout
 * (tests/test_anysize_cpu.py pins that to F.interpolate); GMD_UPSAMPLE_TO(2 Hin, 2 Win) is the launch of upsample=1.  Any other
 * size, and any other value of `upsample` above 1 or below 0, returns GMD_ERR_INVALID before a launch.  The same values hold for
 * gmd_conv3x3_gn_fusable (which answers 0) and gmd_conv3x3_groupnorm.
 * Epilogue as gmd_gemm_nt (rowbias is [B, ldrb], one row per sample; alpha scales the
 * accumulated sum before the bias: 1 for a plain convolution, 2^-s for a weight that was stored scaled by 2^s).  Cin % 64 == 0 (BF16 / F16), % 32 (F32S / F32SW), % 16 (F32). */
#define GMD_UPSAMPLE_TO(Hout, Wout) (((int)(Hout) << 16) | (int)(Wout)) /* 1 <= Hout < 32768, 1 <= Wout < 65536 */
int gmd_conv3x3(const void* X, const void* Wt, void* Y, int dtype, int out_dtype,
                int B, int Hin, int Win, int Cin, int Cout, int stride, int upsample, int pad_mode,
                const float* bias, const float* rowbias, int64_t ldrb, const void* residual, float alpha,
                float* colstats, int colstats_bucket,
                void* workspace, int64_t workspace_bytes, gmd_stream_t stream);

/* gmd_conv3x3 with a K TAIL (added within ABI v14: one new entry point, no signature changed): behind the nine taps over the Cin
 * channels of X the contraction goes on over K2 channels of a second operand X2, row-major [B*Hin*Win, ldx2] (ldx2 >= K2, a multiple
 * of 8) and read at the output pixel itself -- a 1x1 tap:
 *     Y = alpha * (conv3x3(X, Wt[:, :9 Cin]) + X2 Wt[:, 9 Cin:]^T) + bias + rowbias + residual,    Wt: ONE matrix [Cout, 9*Cin + K2].
 * This is diffusers' ResnetBlock2D tail, conv2(h) + conv_shortcut(x), as one launch: the shortcut projection is K2/64 more steps of
 * the K loop that already owns the output tile, summed in the float32 accumulator (the two-launch form rounds the shortcut to 16
 * bits first), and its [M, Cout] tensor is neither written nor read back as `residual`.  The caller packs [W2 | Wsc] and adds the
 * two biases.  16-bit dtypes, stride 1, no upsampling, pad_mode 0, K2 % 64 == 0: anything else returns GMD_ERR_INVALID before a
 * launch, and so does a launch whose plan is not the 256-row ping-pong kernel (or its patch-resident form) (gmd_gemm_plan_info with K = 9*Cin + K2 answers
 * {256, 160 | 128, 283, .}: ask it first and issue gmd_gemm_nt + gmd_conv3x3 otherwise).  Epilogue, column statistics, out_dtype
 * and workspace exactly as gmd_conv3x3; split-K plans (either reduction) slice the 9*Cin/64 + K2/64 steps as one K. */
int gmd_conv3x3_tail(const void* X, const void* X2, const void* Wt, void* Y, int dtype, int out_dtype,
                     int B, int Hin, int Win, int Cin, int K2, int64_t ldx2, int Cout, int stride, int upsample, int pad_mode,
                     const float* bias, const float* rowbias, int64_t ldrb, const void* residual, float alpha,
                     float* colstats, int colstats_bucket,
                     void* workspace, int64_t workspace_bytes, gmd_stream_t stream);

/* gmd_conv3x3 of the nearest-2x upsampled image (upsample = 1, Hout = 2 Hin, Wout = 2 Win) as FOUR 2x2 PHASE CONVOLUTIONS over the
 * low-resolution image (added within ABI v14: two new entry points, no signature changed).  Output pixel (2i + py, 2j + px) reads
 * only the 2x2 window of source pixels (i + a + py - 1, j + b + px - 1), a, b in {0, 1}: the nine taps collapse to four whose
 * weights are sums of the taps that hit the same source pixel -- py = 0: {W[ky=0], W[ky=1] + W[ky=2]}, py = 1: {W[ky=0] + W[ky=1],
 * W[ky=2]}, the same in x -- so K = 4 Cin instead of 9 Cin.  Wp: [4][Cout][4 Cin], phase 2 py + px, tap-major (a, b) inside a phase,
 * summed in float32 and rounded once (the caller packs it once per model).  Zero padding is that of the nine-tap form.  One launch
 * covers the four phases; Y, bias, rowbias ([B, ldrb]), residual, column statistics (blocks of a sample contiguous, B * 4 Hin Win / 64
 * of them as for gmd_conv3x3), out_dtype and workspace as gmd_conv3x3 (alpha = 1).  Only the 256-row ping-pong kernel has the phase
 * loader: gmd_conv3x3_up2_plan answers 1 (and out4 = {256, 160 | 128, 283, K slices}, out4 may be NULL) exactly where the launch is
 * taken -- 16-bit dtype, Cin % 64 == 0, that plan under the calling thread's plan family for M = 4 ceil(B Hin Win / 256) 256,
 * K = 4 Cin, and with colstats_bucket > 0 also Hin Win % 64 == 0 and whole buckets per 80- / 64-column wave tile; otherwise
 * gmd_conv3x3_up2 returns GMD_ERR_UNSUPPORTED and the caller issues gmd_conv3x3(.., upsample = 1, ..) with the nine-tap weight. */
int gmd_conv3x3_up2_plan(int dtype, int B, int Hin, int Win, int Cin, int Cout, int colstats_bucket, int64_t workspace_bytes, int* out4);
int gmd_conv3x3_up2(const void* X, const void* Wp, void* Y, int dtype, int out_dtype,
                    int B, int Hin, int Win, int Cin, int Cout,
                    const float* bias, const float* rowbias, int64_t ldrb, const void* residual,
                    float* colstats, int colstats_bucket,
                    void* workspace, int64_t workspace_bytes, gmd_stream_t stream);

/* conv3x3 whose output goes straight into a GroupNorm (+SiLU): ResnetBlock2D's conv1 -> (+ time embedding) -> norm2 -> SiLU
 * (diffusers ResnetBlock2D.forward; reached through UNet2DConditionModel at stable_diffusion_dual_unet.py:1052, 1083).  On the
 * 16x16 / 8x8 UNet levels the convolution runs split-K (float32 partial slabs in `workspace`); here the GroupNorm kernel sums
 * the slabs itself, applies the convolution's epilogue (alpha, bias, rowbias, residual), rounds to the activation type exactly
 * as the stored tensor would be rounded and normalises from registers: one launch instead of reduce + GroupNorm, the raw
 * tensor neither written nor re-read.  Ynorm = GroupNorm(conv(X)) [+ SiLU]; Yraw (NULL to skip) = conv(X) as gmd_conv3x3
 * would store it.  Results are bit-identical to gmd_conv3x3 followed by gmd_groupnorm_fused.
 * dtype: GMD_BF16 / GMD_F16 (tensors of that type) or GMD_F32S / GMD_F32SW (float32 tensors).  Only launches whose plan is
 * split-K and whose (sample, group) slice fits the register-resident GroupNorm fuse: gmd_conv3x3_gn_fusable() returns 1 for
 * exactly those (same arguments; `groups` = GroupNorm groups); for the others gmd_conv3x3_groupnorm returns
 * GMD_ERR_UNSUPPORTED and the caller issues gmd_conv3x3 + a GroupNorm entry point. */
int gmd_conv3x3_gn_fusable(int dtype, int B, int Hin, int Win, int Cin, int Cout, int stride, int upsample, int pad_mode,
                           int groups, int64_t workspace_bytes);
int gmd_conv3x3_groupnorm(const void* X, const void* Wt, void* Yraw, void* Ynorm, int dtype,
                          int B, int Hin, int Win, int Cin, int Cout, int stride, int upsample, int pad_mode,
                          const float* bias, const float* rowbias, int64_t ldrb, const void* residual, float alpha,
                          int groups, float eps, const float* gamma, const float* beta, int silu,
                          void* workspace, int64_t workspace_bytes, gmd_stream_t stream);

/* Flash-style attention, bf16 MFMA: O = softmax(scale * Q K^T) V per (batch, head).
 * Q: [B,Nq,*] head h at columns h*D..h*D+D, row stride ldq; K likewise (ldk);
 * Vt: V transposed, [B, H*D, ldvt] (keys contiguous, ldvt >= Nk, multiple of 8);
 * O: [B,Nq,H*D] row stride ldo.  D in {32,40,64,80,160}.
 * D = 40, GMD_BF16: one softmax stabiliser per query row (the maximum of its first 64 keys), never updated -- bfloat16 has
 * float32's exponent range; a row whose sum leaves [0, 2^120) re-runs its block maximum-first.  GMD_ATTN40_FIXED=0 in the
 * environment (read once per process) selects the per-tile lagged stabiliser that GMD_F16 always uses: the A/B switch. */
int gmd_attention(const void* Q, const void* K, const void* Vt, void* O, int dtype,
                  int B, int H, int D, int Nq, int Nk,
                  int64_t ldq, int64_t ldk, int64_t ldvt, int64_t ldo,
                  int64_t strideQ, int64_t strideK, int64_t strideVt, int64_t strideO,
                  float scale, int causal, gmd_stream_t stream);
/* Decoupled cross-attention of an IP-Adapter as one launch (added within ABI v14; csrc/attention_ip.hip), GMD_BF16 / GMD_F16:
 *   O = softmax(scale Q K^T) V  +  ip_scale[ip_scale_index] * softmax(scale Q Kip^T) Vip
 * Two INDEPENDENT softmaxes (a maximum and a row sum each); Q is read once, O stored once (one rounding), nothing in between reaches
 * global memory.  Q, K, Vt, O, D as gmd_attention; Kip [B, Nip, *] (ldkip), Vtip [B, H*D, ldvtip] with 1 <= Nip <= 64 (one key tile),
 * ldvtip >= Nip rounded up to 8.  ip_scale: float32 DEVICE array read by the kernel, so a captured graph serves every scale; the
 * host rewrites it outside a captured graph.  B == 0 or Nq == 0: GMD_OK, nothing written.  float32 tensors compose gmd_attention
 * twice and gmd_scaled_add.  reference: IPAdapterAttnProcessor of diffusers, as installed by load_ip_adapter
 * (stable_diffusion_dual_unet.py:518-585). */
int gmd_attention_ip(const void* Q, const void* K, const void* Vt, const void* Kip, const void* Vtip, void* O, int dtype,
                     int B, int H, int D, int Nq, int Nk, int Nip,
                     int64_t ldq, int64_t ldk, int64_t ldvt, int64_t ldkip, int64_t ldvtip, int64_t ldo,
                     int64_t strideQ, int64_t strideK, int64_t strideVt, int64_t strideKip, int64_t strideVtip, int64_t strideO,
                     float softmax_scale, const float* ip_scale, int ip_scale_index, gmd_stream_t stream);
/* causal != 0 (needs Nq == Nk): query q attends keys 0..q only -- the CLIP text encoder's mask
 * (transformers CLIPTextModel, used through stable_diffusion_gm.py:398-439). */

/* row softmax: P[r, :cols] = softmax(scale * S[r, :cols]); S float32 ld lds, P out_dtype ld ldp;
 * columns cols..ldp-1 of P are zero-filled.  causal_nq > 0: row r belongs to query r % causal_nq and
 * columns beyond that query get probability 0. */
int gmd_softmax_rows(const float* S, int64_t lds, void* P, int out_dtype, int64_t ldp,
                     int64_t rows, int cols, float scale, int causal_nq, gmd_stream_t stream);

/* GroupNorm statistics over channels-last X [B,HW,C] -> per (b,c) affine
 * scale_shift[b][c] = {rstd*gamma[c], beta[c]-mean*rstd*gamma[c]}.
 * workspace: float32, at least B*nsplit*G*2 floats where nsplit = gmd_groupnorm_nsplit(HW).  Every one of these B*nsplit*G*2
 * floats is written by each launch (workspace[b][split][g] = {sum, sumsq} of that block's rows; a block whose row range is empty
 * stores zeros) and nothing is read before it is written, so the buffer may hold anything on entry; no float beyond them is touched. */
int gmd_groupnorm_nsplit(int64_t HW);
int gmd_groupnorm_stats(const void* X, int dtype, int B, int64_t HW, int C, int G, float eps,
                        const float* gamma, const float* beta, float* workspace,
                        float* scale_shift, gmd_stream_t stream);
/* Y = [silu](X*scale+shift) */
/* GroupNorm(+SiLU) in two launches for slabs too large for gmd_groupnorm_fused: partial sums per (sample, row split, group)
 * into `workspace` (same size as for gmd_groupnorm_stats), then an apply kernel whose workgroups fold the partials of their
 * sample themselves (deterministic order) -- no separate finalize launch, no scale_shift tensor. */
int gmd_groupnorm_split(const void* X, void* Y, int dtype, int B, int64_t HW, int C, int G, float eps,
                        const float* gamma, const float* beta, float* workspace, int silu, gmd_stream_t stream);
int gmd_groupnorm_apply(const void* X, void* Y, int dtype, int B, int64_t HW, int C,
                        const float* scale_shift, int silu, gmd_stream_t stream);
/* GroupNorm(+SiLU) in ONE pass over X, with the statistics its producer(s) left (`colstats` of gmd_gemm_nt / gmd_conv3x3,
 * one row block per 64 rows: HW % 64 == 0).  X may be the channel concatenation of two producers' outputs (UNet skip
 * connections): channels [0, Ca) use stats_a [B*HW/64][Ca/bucket][2], channels [Ca, C) stats_b [B*HW/64][(C-Ca)/bucket][2]
 * (NULL when Ca == C).  bucket must divide C/G, Ca and C-Ca. */
int gmd_groupnorm_colstats(const void* X, void* Y, int dtype, int B, int64_t HW, int C, int G, float eps,
                           const float* gamma, const float* beta, const float* stats_a, int Ca,
                           const float* stats_b, int bucket, int silu, gmd_stream_t stream);
/* GroupNorm(+SiLU) in ONE launch: one workgroup per (sample, group) over the group's [HW][C/G] slab (exact two-pass
 * variance, fixed reduction order; the slab is re-read from L2).  Returns GMD_ERR_UNSUPPORTED when the slab exceeds
 * 128 KiB: use gmd_groupnorm_stats + gmd_groupnorm_apply then. */
int gmd_groupnorm_fused(const void* X, void* Y, int dtype, int B, int64_t HW, int C, int G, float eps,
                        const float* gamma, const float* beta, int silu, gmd_stream_t stream);
/* LayerNorm over the last dim (C % 8 == 0, C <= 2048) */
int gmd_layernorm(const void* X, void* Y, int dtype, int64_t rows, int C,
                  const float* gamma, const float* beta, float eps, gmd_stream_t stream);
/* GEGLU: Y[r, f] = X[r, f] * gelu_erf(X[r, F + f]); X [rows, 2F], Y [rows, F] */
int gmd_geglu(const void* X, void* Y, int dtype, int64_t rows, int F, gmd_stream_t stream);
/* gmd_geglu over the column layout an interleaved GEGLU projection weight produces (added within ABI v14): value columns of outputs
 * 16 j .. 16 j + 15 at X columns 32 j .. 32 j + 15, their gates at 32 j + 16 .. 32 j + 31.  F % 16 == 0. */
int gmd_geglu_interleaved(const void* X, void* Y, int dtype, int64_t rows, int F, gmd_stream_t stream);
/* sinusoidal timestep embedding (diffusers get_timestep_embedding): out [B, dim] of `dtype`;
 * timestep read from DEVICE memory (t_dev, float32 scalar) so captured graphs can be replayed. */
int gmd_timestep_embedding(const float* t_dev, void* out, int dtype, int B, int dim,
                           int flip_sin_to_cos, float freq_shift, gmd_stream_t stream);
/* gmd_timestep_embedding plus a per-row addend [B, dim] of `dtype` (added within ABI v14): the time embedding input of a
 * guidance-embedded UNet (diffusers' time_embedding.cond_proj: t_emb.to(dtype) + cond_proj(timestep_cond), then linear_1):
 *   out[b, j] = round_dtype( float(round_dtype(sinusoid[b, j])) + float(addend[b, j]) ).  out must not alias addend. */
int gmd_timestep_embedding_add(const float* t_dev, const void* addend, void* out, int dtype, int B, int dim,
                               int flip_sin_to_cos, float freq_shift, gmd_stream_t stream);
/* out[r, :Ca] = A[r], out[r, Ca:] = Bm[r]  (skip-connection concat, channels-last) */
int gmd_concat_channels(const void* A, int Ca, const void* Bm, int Cb, void* out, int dtype,
                        int64_t rows, gmd_stream_t stream);
/* The skip-connection concat with ControlNet residuals added where the skip is read (added within ABI v14; csrc/controlnet.hip):
 *   out[r, :Ca] = Ra ? rnd(A[r]  + rnd(Ra[r - r_row0] * scales[ia])) : A[r]
 *   out[r, Ca:] = Rb ? rnd(Bm[r] + rnd(Rb[r - r_row0] * scales[ib])) : Bm[r]        (rows r < r_row0: plain copy)
 * rnd = one rounding to `dtype`; product and sum in float32 and never contracted: bit for bit torch's `s + r * scale` on tensors of
 * `dtype` with a float32 scalar.  Ra [rows - r_row0, Ca] / Rb [rows - r_row0, Cb] of `dtype`, either may be NULL (that part is then a
 * copy).  scales: float32 DEVICE array of 13 entries read by the kernel (ia, ib in [0, 13)); the host rewrites it outside a captured
 * graph.  r_row0 in [0, rows]: the residuals cover the rows from r_row0 on (guess mode: the conditional half of a guidance batch).
 * Alignment and channel multiples as gmd_concat_channels (16-byte pointers, Ca and Cb multiples of 8 (16-bit) / 4 (float32)).
 * colstats_b (may be NULL): the launch also writes float32 [rows/64][Cb/colstats_bucket][2] = {sum, sum of squares} of the STORED
 * B-part outputs in a fixed order (32 + 2 + bucket float32 additions per entry, as the producers' row epilogue): the stats_b operand
 * of gmd_groupnorm_colstats.  Needs rows % 64 == 0, Cb % colstats_bucket == 0, Cb <= 4096 (and, for the consumer, a sample's rows a
 * multiple of 64).  Anything else returns GMD_ERR_INVALID before a launch. */
int gmd_concat_channels_add(const void* A, int Ca, const void* Ra, int ia, const void* Bm, int Cb, const void* Rb, int ib,
                            const float* scales, int64_t r_row0, void* out, int dtype, int64_t rows,
                            float* colstats_b, int colstats_bucket, gmd_stream_t stream);
/* The skip-connection concat of one FreeU site (diffusers' enable_freeu) in ONE launch (added within ABI v14: one new entry point, no
 * signature changed; csrc/freeu.hip), channels-last, GMD_F32 / GMD_BF16 / GMD_F16:
 *   out[r, 0 : Ca/2]     = rnd(float(A[r, c]) * params[ib])
 *   out[r, Ca/2 : Ca]    = A[r, c]
 *   out[r, Ca : Ca + Cs] = rnd(float(S[r, c]) + (params[is] - 1) * low_{b,c}[y, x]),      row r = (b * H + y) * W + x
 * low = the real part of the inverse transform of the skip's bins {0, -1} x {0, -1} (an axis of length 1: {0} alone; of length 2: both
 * of its bins): diffusers' fourier_filter with threshold = 1 (the only value it passes) is X + (scale - 1) * low.  With th_y = 2 pi y / H,
 * ph_x = 2 pi x / W and (u, v) over {0, 1}^2 (u = 1 only for H > 1, v = 1 only for W > 1):
 *   c_uv = sum_{y,x} X cos(u th_y + v ph_x),  d_uv = sum_{y,x} X sin(u th_y + v ph_x)
 *   low[y, x] = 1 / (H W) * sum_{u,v} (c_uv cos(u th_y + v ph_x) + d_uv sin(u th_y + v ph_x))
 * All arithmetic in float32, rnd = ONE rounding to `dtype`.  The backbone half is bit for bit torch's `h * b` on a tensor of `dtype`
 * with a float32 scalar; params[is] == 1 / params[ib] == 1 make that part a raw copy.
 *   A [B*H*W, Ca] with row stride lda, S [B*H*W, Cs] with row stride lds, out with row stride ldo >= Ca + Cs (strides in elements)
 *   params: float32 DEVICE array read by the kernel (the convention of gmd_scaled_add / gmd_lora_update: one captured graph serves every
 *           setting); ib / is index it
 * In place: out may be the buffer A and S are views of -- A == out, S == out + Ca, lda == lds == ldo (behind gmd_concat_channels_add:
 * the filter must see skip + ControlNet residual).  Every element is read for the last time and written by the same lane, and all reads
 * that feed a channel's coefficients complete before one of its elements is overwritten.  No atomics; the summation order depends on
 * (H, W) only, so a sample's output is the same bits whatever else is in the launch.  Nothing outside rows [0, B*H*W) x columns
 * [0, Ca + Cs) is written.  B == 0: GMD_OK, nothing written.
 * GMD_ERR_INVALID before a launch: pointers not 16-byte aligned; Ca / 2, Cs or a stride not a multiple of 8 (16-bit) / 4 (float32); a
 * stride smaller than its row; H < 1 or W < 1; a NULL params or a negative index; a tensor beyond 2 GiB (32-bit byte offsets); A / S /
 * out overlapping in any way other than the in-place form; H + W above 800 (16-bit) / 4496 (float32): the phase tables share the
 * workgroup's 64 KB of LDS with the partial sums.  Not built: a threshold other than 1, the FreeU authors' "v2" backbone map. */
int gmd_concat_channels_freeu(const void* A, int Ca, int64_t lda, const void* S, int Cs, int64_t lds, void* out, int64_t ldo,
                              int dtype, int B, int H, int W, const float* params, int ib, int is, gmd_stream_t stream);
/* X[i] = X[i] * sigmoid(X[i]) in place, n elements (a multiple of 8 (16-bit) / 4 (float32)), with the formula of the GroupNorm + SiLU
 * kernels (hardware reciprocal of 1 + exp(-x), float32 inside, one rounding on the store).  The ControlNet conditioning embedding's
 * activations, once per call (added within ABI v14). */
int gmd_silu(void* X, int dtype, int64_t n, gmd_stream_t stream);
/* out[r, :] = table[ids[r], :] + pos[r % T, :]  (token + position embedding of the CLIP text encoder,
 * stable_diffusion_gm.py:398-439); ids int32 in [0, vocab) -- out-of-range ids are an error the HOST must
 * exclude (checked there), rows = B*T. */
int gmd_embedding_lookup(const int32_t* ids, const void* table, const void* pos, void* out, int dtype,
                         int64_t rows, int T, int C, int vocab, gmd_stream_t stream);
/* out[0:bytes] = out[bytes:2*bytes] = in[0:bytes] (bytes % 16 == 0): the batch duplication of classifier-free guidance
 * (stable_diffusion_dual_unet.py:1045-1047 torch.cat([latents] * 2)) applied to an activation where the two conditionings
 * first differ (the CFG shared prefix of UNet2DConditionModel.forward_packed) */
int gmd_dup_batch(const void* in, void* out, int64_t bytes, gmd_stream_t stream);
/* out[i] = a[i] + b[i] * scales[index], n elements (a multiple of 8 (16-bit) / 4 (float32)), float32 inside, one rounding on the
 * store; scales is a float32 DEVICE array.  out may alias a.  The combine of the composed decoupled cross-attention (added within
 * ABI v14). */
int gmd_scaled_add(const void* a, const void* b, void* out, int dtype, int64_t n, const float* scales, int index, gmd_stream_t stream);
/* A LoRA adapter applied at run time (added within ABI v14: one new entry point, no signature changed; csrc/lora.hip), GMD_BF16 /
 * GMD_F16: the rank update of a projection's output as ONE launch,
 *   Y[m, n] <- round( float(Y[m, n]) + scales[index] * sum_j T[m, j] * Bw[n, j] ),   T[m, j] = round( sum_k X[m, k] * Aw[j, k] )
 * Both sums in float32 on the matrix cores, T rounded ONCE to `dtype` between them (what a 16-bit PEFT model does between lora_A and
 * lora_B), the scale applied in float32 to the second sum, one rounding on the store.
 *   X  [M, K], row stride ldx (>= K), K % 64 == 0;   Aw [Rp, K];   Bw [N, Rp]
 *   Rp: the rank zero-padded by the host to a multiple of 32, at most 128 (true ranks 1..128)
 *   transposed == 0: Y [M, N], row stride ldy >= N, N % 8 == 0 (ldy > N: a column range of a wider buffer, through a pointer offset);
 *                    batch / tokens / strideY are ignored
 *   transposed != 0: Y [batch, N, ldy] with the token contiguous (a V^T: gmd_gemm_qkv_vt's second output, the cached cross-attention
 *                    vt), M == batch * tokens, row m = b * tokens + tok lands at Y[b * strideY + n * ldy + tok]; ldy >= tokens rounded
 *                    up to 8, strideY >= N * ldy
 * Nothing outside rows [0, M) x columns [0, N) -- transposed: tokens [0, tokens) of each row -- is written; every element is written by
 * exactly one lane, once (no atomics), and a row's result does not depend on what else is in the launch.  scales: float32 DEVICE array
 * read by the kernel (the convention of gmd_scaled_add), so a captured graph serves every scale.  M == 0: GMD_OK, nothing written.
 * GMD_ERR_INVALID before a launch: X overlapping Y, pointers not 16-byte aligned, ldx / ldy / strideY not multiples of 8, K % 64,
 * Rp % 32, Rp > 128, a NULL scales, X or one batch entry of Y beyond 2 GiB (32-bit byte offsets through buffer descriptors).
 * GMD_F32 and the split dtypes: GMD_ERR_UNSUPPORTED (the caller composes gmd_gemm_nt twice and gmd_scaled_add). */
int gmd_lora_update(const void* X, const void* Aw, const void* Bw, void* Y, int dtype, int M, int K, int Rp, int N,
                    int64_t ldx, int64_t ldy, int transposed, int batch, int tokens, int64_t strideY,
                    const float* scales, int index, gmd_stream_t stream);
/* The LoRA update of a feed-forward's first projection (ff.net.0.proj) and its GEGLU as ONE launch (added within ABI v14: one new
 * entry point, no signature changed; csrc/lora.hip), GMD_BF16 / GMD_F16:
 *   F[m, f] = round( v * gelu_erf(g) ),   v = float(Y[m, value(f)]) + s U[m, value(f)],   g = float(Y[m, gate(f)]) + s U[m, gate(f)]
 *   U[m, n] = sum_j T[m, j] * Bw[n, j],   T[m, j] = round( sum_k X[m, k] * Aw[j, k] ),    s = scales[index]
 * The arithmetic of gmd_lora_update (both sums in float32 on the matrix cores, T rounded ONCE, the scale in float32); v, g, the erf
 * GELU of gmd_geglu and the product stay in float32, ONE rounding on the store of F.
 *   X  [M, C], row stride ldx: the feed-forward's input (the LayerNorm output), C % 64 == 0;   Aw [Rp, C];   Bw [8C, Rp]
 *   Y  [M, 8C], row stride ldy, READ-ONLY: the pre-activation (gmd_gemm_nt with the bias, GMD_ACT_NONE) over the ROW-INTERLEAVED ff1
 *      weight, so its columns are interleaved in groups of 16 (gmd_geglu_interleaved): value(f) = 32 (f / 16) + f % 16,
 *      gate(f) = value(f) + 16.  Bw's rows are in that same order (the host permutes them once).
 *   F  [M, 4C], row stride ldf: every element of rows [0, M) x columns [0, 4C) is written once by one lane, nothing else is
 *   Rp, scales, index: as gmd_lora_update.  A row's result does not depend on what else is in the launch.  M == 0: GMD_OK.
 * GMD_ERR_INVALID before a launch: F overlapping X or Y, pointers not 16-byte aligned, leading dimensions not multiples of 8 or too
 * small, C % 64, Rp % 32, Rp > 128, a NULL scales, X / Y / F beyond 2 GiB.  GMD_F32 and the split dtypes: GMD_ERR_UNSUPPORTED (the
 * caller composes gmd_gemm_nt twice, gmd_scaled_add and gmd_geglu / gmd_geglu_interleaved). */
int gmd_lora_geglu(const void* X, const void* Aw, const void* Bw, const void* Y, void* F, int dtype, int M, int C, int Rp,
                   int64_t ldx, int64_t ldy, int64_t ldf, const float* scales, int index, gmd_stream_t stream);
/* SEVERAL LoRA adapters on one projection as ONE launch (added within ABI v14: two new entry points, no signature changed;
 * csrc/lora.hip), GMD_BF16 / GMD_F16.  Operands, modes and checks of gmd_lora_update / gmd_lora_geglu, except:
 *   Aw [Rp, K], Bw [N, Rp]: the adapters' factors side by side along the rank; the SUM of the ranks zero-padded to a multiple of 32,
 *                           Rp in {32, 64, ..., 256}
 *   colscales, index, ldc:  a float32 DEVICE table with row stride ldc >= Rp; the launch reads the Rp column scales of row `index`
 *   T[m, j]  = round( colscales[index * ldc + j] * sum_k X[m, k] * Aw[j, k] )     float32 sum, the scale in float32, ONE rounding
 *   Y[m, n] <- round( float(Y[m, n]) + sum_j T[m, j] * Bw[n, j] )                 float32 sum, one rounding on the store
 *   GEGLU:    v, g as gmd_lora_geglu with U = sum_j T * Bw and no further scale
 * A column whose sum over k is exactly 0 (every zero-padded column) contributes exactly 0 whatever its table entry holds.  Y (or F) is
 * read and written once; the summation orders depend on k and j only, never on the grid; no atomics.
 * GMD_ERR_INVALID also for Rp > 256, a NULL colscales, ldc < Rp, index < 0. */
int gmd_lora_update_stacked(const void* X, const void* Aw, const void* Bw, void* Y, int dtype, int M, int K, int Rp, int N,
                            int64_t ldx, int64_t ldy, int transposed, int batch, int tokens, int64_t strideY,
                            const float* colscales, int index, int64_t ldc, gmd_stream_t stream);
int gmd_lora_geglu_stacked(const void* X, const void* Aw, const void* Bw, const void* Y, void* F, int dtype, int M, int C, int Rp,
                           int64_t ldx, int64_t ldy, int64_t ldf, const float* colscales, int index, int64_t ldc, gmd_stream_t stream);
/* elementwise cast between F32 and BF16 */
int gmd_cast(const void* in, int in_dtype, void* out, int out_dtype, int64_t n, gmd_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GMD_HIP_H */
