// Latent-side kernels of the denoising loop: CFG combine + x0 prediction + PNDM/PLMS update in one
// pass (and its siblings for DPM-Solver++, DDPM, DDIM, LCM, Euler, LMS and UniPC), the guidance-rescale std reduction, the img2img start / inpaint blend, and the UNet input pack / output unpack (8-channel
// concat + CFG duplicate + NCHW<->channels-last + cast + channel padding).
//
// Built with -ffp-contract=off: float32 operations are issued in the same order as the torch
// expressions of the reference so the results are bit-identical to the CPU path given identical eps.
#include "gmd_common.h"

#include <cmath>
#include <cstdint>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;

// What every step kernel starts from: the UNet's raw output (both halves of the CFG pair when do_cfg: [2B, chw]), the sample, the
// shape and the guidance scalars.  ratio: cfg_std_ratio_kernel's per-sample std ratio, nullptr = no guidance rescale.  The output
// pointers and the schedulers' own inputs stay __restrict__ kernel parameters.
struct StepIn {
    const float* eps_in;
    const float* x;
    int B;
    int64_t chw;
    int do_cfg;
    float gs;
    const float* ratio;
    float gr;
};

// The guided eps of element i: the CFG combine with rescale_noise_cfg, or the plain load.
__device__ __forceinline__ float guided_eps(const StepIn& in, int64_t i, int64_t n) {
    float eps;
    if (in.do_cfg) {
        const float u = in.eps_in[i], t = in.eps_in[n + i];
        eps = u + in.gs * (t - u);  // dual.py:1065
        if (in.ratio) {             // rescale_noise_cfg, dual.py:91-93
            const float resc = eps * in.ratio[i / in.chw];
            eps = in.gr * resc + (1.0f - in.gr) * eps;
        }
    } else {
        eps = in.eps_in[i];
    }
    return eps;
}

// The pipeline's own x0 (dual.py:1075), from alphas_cumprod[t] of the loop timestep; never clipped.
__device__ __forceinline__ float pipeline_x0(float xt, float eps, float sqrt_a, float sqrt_1ma) { return (xt - sqrt_1ma * eps) / sqrt_a; }

// The grid-stride loop of every step kernel: update(i, eps, xt) with the guided eps and the sample of element i.  The block size is
// read by the builtin: blockDim.x is folded into a scalar load of the dispatch's block size only in a kernel's own body, and costs a
// vector load in front of the loop when read in a device function.
template <typename Update>
__device__ __forceinline__ void for_each_guided(const StepIn& in, Update update) {
    GMD_WG_TRACE_SCOPE(WGK_LATENT_STEP);
    const unsigned threads = __builtin_amdgcn_workgroup_size_x();
    const int64_t stride = (int64_t)gridDim.x * threads;
    const int64_t n = (int64_t)in.B * in.chw;
    for (int64_t i = (int64_t)blockIdx.x * threads + threadIdx.x; i < n; i += stride) {
        const float eps = guided_eps(in, i, n);
        const float xt = in.x[i];
        update(i, eps, xt);
    }
}

__global__ __launch_bounds__(kThreads) void latent_step_kernel(
    StepIn in, const float* __restrict__ cur_sample, const float* __restrict__ e1, const float* __restrict__ e2,
    const float* __restrict__ e3, int mode, float sample_coeff, float alpha_delta, float denom, float sqrt_a, float sqrt_1ma,
    float* __restrict__ eps_out, float* __restrict__ x_prev, float* __restrict__ x0) {
    for_each_guided(in, [=](int64_t i, float eps, float xt) {
        if (eps_out) eps_out[i] = eps;
        if (x0) x0[i] = pipeline_x0(xt, eps, sqrt_a, sqrt_1ma);
        float m, smp = xt;
        switch (mode) {  // diffusers PNDMScheduler.step_plms
            case 0: m = eps; break;
            case 1: m = (eps + e1[i]) / 2.0f; smp = cur_sample[i]; break;
            case 2: m = (3.0f * eps - e1[i]) / 2.0f; break;
            case 3: m = (23.0f * eps - 16.0f * e1[i] + 5.0f * e2[i]) / 12.0f; break;
            default: m = (1.0f / 24.0f) * (55.0f * eps - 59.0f * e1[i] + 37.0f * e2[i] - 9.0f * e3[i]); break;
        }
        x_prev[i] = sample_coeff * smp - alpha_delta * m / denom;  // _get_prev_sample
    });
}

// DPM-Solver++ (dpmsolver++ / midpoint / epsilon) multistep update fused with the CFG combine and both x0 forms, in the
// operation order of the torch expressions of diffusers' DPMSolverMultistepScheduler (float32, no FMA contraction):
//   m0     = (x - sigma_s0 * eps) / alpha_s0                                   convert_model_output
//   order1 : x_prev = c_x * x - c_m * m0                                       dpm_solver_first_order_update
//   order2 : x_prev = c_x * x - c_m * m0 - c_h * (inv_r0 * (m0 - m1))          multistep_dpm_solver_second_order_update
// with c_x = sigma_t/sigma_s0, c_m = alpha_t*(exp(-h)-1), c_h = 0.5*c_m computed by the host in float32.
__global__ __launch_bounds__(kThreads) void dpm_step_kernel(
    StepIn in, const float* __restrict__ m1, int order, float sigma_s0, float alpha_s0, float c_x, float c_m, float c_h, float inv_r0,
    float sqrt_a, float sqrt_1ma, float* __restrict__ m0_out, float* __restrict__ x_prev, float* __restrict__ x0) {
    for_each_guided(in, [=](int64_t i, float eps, float xt) {
        if (x0) x0[i] = pipeline_x0(xt, eps, sqrt_a, sqrt_1ma);
        const float m0 = (xt - sigma_s0 * eps) / alpha_s0;
        m0_out[i] = m0;
        float r = c_x * xt - c_m * m0;
        if (order == 2) r = r - c_h * (inv_r0 * (m0 - m1[i]));
        x_prev[i] = r;
    });
}

// SDE-DPM-Solver++ ("DPM++ 2M SDE": algorithm_type "sde-dpmsolver++", midpoint or heun, epsilon) multistep update fused with the
// CFG combine and both x0 forms, in the operation order of the torch expressions of diffusers' DPMSolverMultistepScheduler
// (float32, no FMA contraction):
//   m0     = (x - sigma_s0 * eps) / alpha_s0                                           convert_model_output
//   order1 : x_prev = c_x * x + c_m * m0 + c_n * noise                                 dpm_solver_first_order_update
//   order2 : x_prev = c_x * x + c_m * m0 + c_h * (inv_r0 * (m0 - m1)) + c_n * noise    multistep_dpm_solver_second_order_update
// with c_x = sigma_t/sigma_s0*exp(-h), c_m = alpha_t*(1-exp(-2h)), c_n = sigma_t*sqrt(1-exp(-2h)) and c_h = 0.5*c_m (midpoint) or
// alpha_t*((1-exp(-2h))/(-2h)+1) (heun), computed by the host in float32.  The noise is added at every step, also with c_n == 0
// (the last step of a final_sigmas_type "zero" schedule): torch adds the zero product there too, and -0.0 + 0.0 is not -0.0.  It
// is drawn by the HOST scheduler, as for DDPM and DDIM.
__global__ __launch_bounds__(kThreads) void dpm_sde_step_kernel(
    StepIn in, const float* __restrict__ m1, const float* __restrict__ noise, int order, float sigma_s0, float alpha_s0, float c_x,
    float c_m, float c_h, float inv_r0, float c_n, float sqrt_a, float sqrt_1ma, float* __restrict__ m0_out,
    float* __restrict__ x_prev, float* __restrict__ x0) {
    for_each_guided(in, [=](int64_t i, float eps, float xt) {
        if (x0) x0[i] = pipeline_x0(xt, eps, sqrt_a, sqrt_1ma);
        const float m0 = (xt - sigma_s0 * eps) / alpha_s0;
        m0_out[i] = m0;
        float r = c_x * xt + c_m * m0;
        if (order == 2) r = r + c_h * (inv_r0 * (m0 - m1[i]));
        r = r + c_n * noise[i];
        x_prev[i] = r;
    });
}

// DDPM ancestral step (the scheduler scripts/inference/generate_hdr.py:162 constructs) fused with the CFG combine and the
// pipeline's x0, in the operation order of the torch expressions of diffusers' DDPMScheduler.step (float32, no FMA):
//   x0    = (x - sqrt(1-a_t) * eps) / sqrt(a_t)            [clamped to +-clip_range when clip_sample]
//   prev  = x0_coeff * x0 + xt_coeff * x                    posterior mean, formula (7) of the DDPM paper
//   prev  = prev + noise_scale * noise                      t > 0 only (noise == nullptr at the last step)
// The noise tensor is drawn by the HOST scheduler with randn_tensor(generator) so that the shared generator of the dual
// pipeline is consumed in the reference's order (SDR step first, GM step second: stable_diffusion_dual_unet.py:1077, 1093).
__global__ __launch_bounds__(kThreads) void ddpm_step_kernel(
    StepIn in, const float* __restrict__ noise, float sched_sqrt_a, float sched_sqrt_1ma, int clip, float clip_range, float x0_coeff,
    float xt_coeff, float noise_scale, float sqrt_a, float sqrt_1ma, float* __restrict__ x_prev, float* __restrict__ x0) {
    for_each_guided(in, [=](int64_t i, float eps, float xt) {
        if (x0) x0[i] = pipeline_x0(xt, eps, sqrt_a, sqrt_1ma);
        float p0 = (xt - sched_sqrt_1ma * eps) / sched_sqrt_a;
        if (clip) p0 = fminf(fmaxf(p0, -clip_range), clip_range);
        float r = x0_coeff * p0 + xt_coeff * xt;
        if (noise) r = r + noise_scale * noise[i];
        x_prev[i] = r;
    });
}

// DDIM step (the scheduler the pipelines' docstrings name first; `eta` is its dial towards DDPM) fused with the CFG combine
// and the pipeline's x0, in the operation order of the torch expressions of diffusers' DDIMScheduler.step (epsilon
// prediction, float32, no FMA):
//   p0   = (x - sqrt(1-a_t) * eps) / sqrt(a_t)                      pred_original_sample [clamped to +-clip_range]
//   pe   = use_clipped ? (x - sqrt(a_t) * p0) / sqrt(1-a_t) : eps   pred_epsilon
//   prev = sqrt(a_prev) * p0 + dir_coeff * pe                       dir_coeff = (1 - a_prev - std^2) ** 0.5
//   prev = prev + std * noise                                       eta > 0 only (noise == nullptr otherwise)
// The add happens whenever a noise tensor is given, also with std == 0 (the last step of a set_alpha_to_one schedule): torch
// adds the zero product there too, and -0.0 + 0.0 is not -0.0.  The noise is drawn by the HOST scheduler, as for DDPM.
__global__ __launch_bounds__(kThreads) void ddim_step_kernel(
    StepIn in, const float* __restrict__ noise, float sched_sqrt_a, float sched_sqrt_1ma, int clip, float clip_range, int use_clipped,
    float sqrt_a_prev, float dir_coeff, float std, float sqrt_a, float sqrt_1ma, float* __restrict__ x_prev, float* __restrict__ x0,
    float* __restrict__ pred_x0) {
    for_each_guided(in, [=](int64_t i, float eps, float xt) {
        if (x0) x0[i] = pipeline_x0(xt, eps, sqrt_a, sqrt_1ma);
        float p0 = (xt - sched_sqrt_1ma * eps) / sched_sqrt_a;
        if (clip) p0 = fminf(fmaxf(p0, -clip_range), clip_range);
        if (pred_x0) pred_x0[i] = p0;
        const float pe = use_clipped ? (xt - sched_sqrt_a * p0) / sched_sqrt_1ma : eps;
        float r = sqrt_a_prev * p0 + dir_coeff * pe;
        if (noise) r = r + std * noise[i];
        x_prev[i] = r;
    });
}

// Latent-consistency (LCM) step -- diffusers' LCMScheduler.step, epsilon prediction -- fused with the CFG combine and the pipeline's
// x0, in the operation order of its torch expressions (float32, no FMA):
//   p0    = (x - sqrt(1-a_t) * eps) / sqrt(a_t)            predicted_original_sample [clamped to +-clip_range when clip_sample;
//                                                          a NaN passes the clamp as it passes torch.clamp]
//   den   = c_out * p0 + c_skip * x                        the consistency model's "denoised" (boundary-condition scalings)
//   prev  = sqrt(a_prev) * den + sqrt(1-a_prev) * noise    every step but the last (noise == nullptr there: prev = den)
// The noise is drawn by the HOST scheduler, as for DDPM and DDIM.  A guidance-embedded UNet runs without the CFG duplicate, but the
// combine stays available: LCMScheduler also steps a plain UNet.
__global__ __launch_bounds__(kThreads) void lcm_step_kernel(
    StepIn in, const float* __restrict__ noise, float sched_sqrt_a, float sched_sqrt_1ma, int clip, float clip_range, float c_skip,
    float c_out, float sqrt_a_prev, float sqrt_b_prev, float sqrt_a, float sqrt_1ma, float* __restrict__ x_prev,
    float* __restrict__ x0, float* __restrict__ denoised) {
    for_each_guided(in, [=](int64_t i, float eps, float xt) {
        if (x0) x0[i] = pipeline_x0(xt, eps, sqrt_a, sqrt_1ma);
        float p0 = (xt - sched_sqrt_1ma * eps) / sched_sqrt_a;
        if (clip) p0 = p0 < -clip_range ? -clip_range : (p0 > clip_range ? clip_range : p0);  // torch.clamp: a NaN stays a NaN
        const float den = c_out * p0 + c_skip * xt;
        if (denoised) denoised[i] = den;
        x_prev[i] = noise ? sqrt_a_prev * den + sqrt_b_prev * noise[i] : den;
    });
}

// Euler / Euler-ancestral step (diffusers' EulerDiscreteScheduler / EulerAncestralDiscreteScheduler, epsilon prediction, s_churn == 0)
// fused with the CFG combine, in the operation order of their torch expressions (float32, no FMA contraction):
//   p0     = x - sigma_hat * eps            pred_original_sample (also the pipeline's x0: sigma space has no other form)
//   d      = (x - p0) / sigma_hat           derivative
//   x_prev = x + d * dt                     dt = sigma_next - sigma_hat (Euler) or sigma_down - sigma (ancestral)
//   x_prev = x_prev + noise * sigma_up      ancestral only (noise == nullptr otherwise)
// The add happens whenever a noise tensor is given, also with sigma_up == 0 (the last step, sigma_to == 0): torch adds the zero
// product there too, and -0.0 + 0.0 is not -0.0.  The noise is drawn by the HOST scheduler, as for DDPM and DDIM.
__global__ __launch_bounds__(kThreads) void euler_step_kernel(StepIn in, const float* __restrict__ noise, float sigma_hat, float dt,
                                                              float sigma_up, float* __restrict__ x_prev, float* __restrict__ pred_x0) {
    for_each_guided(in, [=](int64_t i, float eps, float xt) {
        const float p0 = xt - sigma_hat * eps;
        if (pred_x0) pred_x0[i] = p0;
        const float d = (xt - p0) / sigma_hat;
        float r = xt + d * dt;
        if (noise) r = r + noise[i] * sigma_up;
        x_prev[i] = r;
    });
}

// Linear multistep step (diffusers' LMSDiscreteScheduler, epsilon prediction, orders 1-4) fused with the CFG combine, in the
// operation order of its torch expressions (float32, no FMA contraction):
//   p0     = x - sigma * eps                pred_original_sample (also the pipeline's x0, as for Euler)
//   d      = (x - p0) / sigma               derivative; stored to d_out: the host keeps it as the next steps' history
//   acc    = 0.0f + c0 * d                  Python's sum() starts from int 0, and 0 + (-0.0) is +0.0: the add is a real one
//   acc    = acc + c1 * d1 [+ c2 * d2 [+ c3 * d3]]      d1, d2, d3: the derivatives of the previous 1, 2, 3 steps
//   x_prev = x + acc
// c0..c3 are the integrals of the Lagrange basis polynomials over [sigma, sigma_next], computed by the host in float64 and rounded
// to float32 once, by the ``float`` argument.  A history pointer beyond order - 1 is never read.
__global__ __launch_bounds__(kThreads) void lms_step_kernel(
    StepIn in, const float* __restrict__ d1, const float* __restrict__ d2, const float* __restrict__ d3, int order, float sigma,
    float c0, float c1, float c2, float c3, float* __restrict__ d_out, float* __restrict__ x_prev, float* __restrict__ pred_x0) {
    for_each_guided(in, [=](int64_t i, float eps, float xt) {
        const float p0 = xt - sigma * eps;
        if (pred_x0) pred_x0[i] = p0;
        const float d = (xt - p0) / sigma;
        d_out[i] = d;
        float acc = 0.0f + c0 * d;
        if (order >= 2) acc = acc + c1 * d1[i];
        if (order >= 3) acc = acc + c2 * d2[i];
        if (order >= 4) acc = acc + c3 * d3[i];
        x_prev[i] = xt + acc;
    });
}

// UniPC predictor-corrector step (Zhao et al. 2023; diffusers' UniPCMultistepScheduler: predict_x0, epsilon prediction, bh1 / bh2,
// orders 1-3) fused with the CFG combine and both x0 forms, in the operation order of the scheduler's torch expressions (float32, no FMA
// contraction).  h1, h2, h3 are the x0 predictions of the previous 1, 2, 3 steps (m0_out of those launches), `last` the x_corr of the
// previous launch:
//   m0     = (x - sigma_s * eps) / alpha_s                          the x0 prediction, from x as it comes in (before the correction)
//   corrector of order p (0 = off: x_corr = x), r_p = 1 so its D is m0 - h1:
//     acc    = c_rho[0] * ((h2 - h1) / c_r1) [+ c_rho[1] * ((h3 - h1) / c_r2)] + c_rho[p-1] * (m0 - h1)     (p = 1: the last term alone)
//     x_corr = c_x * last - c_m * h1 - c_b * acc
//   predictor of order q:
//     x_prev = p_x * x_corr - p_m * m0 [- p_b * (p_rho[0] * ((h1 - m0) / p_r1) [+ p_rho[1] * ((h2 - m0) / p_r2)])]    (q = 1: no p_b term)
// with c_x / p_x = sigma_t/sigma_s, c_m / p_m = alpha_t*phi_1, c_b / p_b = alpha_t*B_h of the two intervals and rho = R^-1 b, all computed
// by the host in float32.  The kernel divides by r_k, as the host expression does.  A pointer or scalar beyond the orders is never read.
__global__ __launch_bounds__(kThreads) void unipc_step_kernel(
    StepIn in, const float* __restrict__ last, const float* __restrict__ h1, const float* __restrict__ h2, const float* __restrict__ h3,
    int corr_order, int pred_order, float sigma_s, float alpha_s, float c_x, float c_m, float c_b, float c_rho1, float c_rho2,
    float c_rho3, float c_r1, float c_r2, float p_x, float p_m, float p_b, float p_rho1, float p_rho2, float p_r1, float p_r2,
    float sqrt_a, float sqrt_1ma, float* __restrict__ m0_out, float* __restrict__ x_corr, float* __restrict__ x_prev,
    float* __restrict__ x0) {
    for_each_guided(in, [=](int64_t i, float eps, float xt) {
        if (x0) x0[i] = pipeline_x0(xt, eps, sqrt_a, sqrt_1ma);
        const float m0 = (xt - sigma_s * eps) / alpha_s;
        m0_out[i] = m0;
        float xc = xt;
        if (corr_order >= 1) {
            const float m1 = h1[i];
            float acc;
            if (corr_order == 1) {
                acc = c_rho1 * (m0 - m1);
            } else {
                acc = c_rho1 * ((h2[i] - m1) / c_r1);
                if (corr_order == 3) acc = acc + c_rho2 * ((h3[i] - m1) / c_r2);
                acc = acc + (corr_order == 3 ? c_rho3 : c_rho2) * (m0 - m1);
            }
            xc = c_x * last[i] - c_m * m1 - c_b * acc;
        }
        x_corr[i] = xc;
        float r = p_x * xc - p_m * m0;
        if (pred_order >= 2) {
            float acc = p_rho1 * ((h1[i] - m0) / p_r1);
            if (pred_order == 3) acc = acc + p_rho2 * ((h2[i] - m0) / p_r2);
            r = r - p_b * acc;
        }
        x_prev[i] = r;
    });
}

// one block per sample: unbiased std over chw of text eps and of the guided eps
__global__ __launch_bounds__(kThreads) void cfg_std_ratio_kernel(const float* __restrict__ eps_in, int B, int64_t chw,
                                                                 float gs, float* __restrict__ ratio) {
    GMD_WG_TRACE_SCOPE(WGK_CFG_RATIO);
    const int b = blockIdx.x;
    const int64_t n = (int64_t)B * chw;
    const float* u = eps_in + (int64_t)b * chw;
    const float* t = eps_in + n + (int64_t)b * chw;
    double st = 0, st2 = 0, sc = 0, sc2 = 0;
    for (int64_t i = threadIdx.x; i < chw; i += blockDim.x) {
        const float tv = t[i], uv = u[i];
        const float cv = uv + gs * (tv - uv);
        st += tv; st2 += (double)tv * tv; sc += cv; sc2 += (double)cv * cv;
    }
    __shared__ double red[4][kThreads];
    red[0][threadIdx.x] = st; red[1][threadIdx.x] = st2; red[2][threadIdx.x] = sc; red[3][threadIdx.x] = sc2;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o)
            for (int k = 0; k < 4; ++k) red[k][threadIdx.x] += red[k][threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double N = (double)chw;
        const double vt = (red[1][0] - red[0][0] * red[0][0] / N) / (N - 1.0);
        const double vc = (red[3][0] - red[2][0] * red[2][0] / N) / (N - 1.0);
        ratio[b] = (float)sqrt(vt) / (float)sqrt(vc);  // float32 std values, float32 division
    }
}

// kScaled: each source is divided by its own float32 divisor before the one rounding to T (a sigma-space scheduler's
// scale_model_input, sample / ((sigma**2 + 1) ** 0.5): a float32 division, not a reciprocal multiply); padding channels stay zero.
// The plain instantiation holds no division and ignores div0 / div1.
template <typename T, bool kScaled>
__global__ __launch_bounds__(kThreads) void pack_kernel(const float* __restrict__ s0, int C0, float div0, const float* __restrict__ s1,
                                                        int C1, float div1, int B, int64_t HW, int dup, T* __restrict__ out, int CP) {
    GMD_WG_TRACE_SCOPE(WGK_PACK);
    // one thread per (pixel, 8-channel group) of the padded output
    const int groups = CP / 8;
    const int64_t total = (int64_t)B * HW * groups;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int g = (int)(i % groups);
        const int64_t bp = i / groups;
        const int64_t b = bp / HW, p = bp - b * HW;
        float v[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int c = g * 8 + j;
            float val = 0.0f;
            if (c < C0) {
                val = s0[(b * C0 + c) * HW + p];
                if (kScaled) val = val / div0;
            } else if (c < C0 + C1) {
                val = s1[(b * C1 + (c - C0)) * HW + p];
                if (kScaled) val = val / div1;
            }
            v[j] = val;
        }
        for (int d = 0; d < dup; ++d) {
            T* o = out + (((int64_t)d * B + b) * HW + p) * CP + g * 8;
#pragma unroll
            for (int j = 0; j < 8; ++j) Elem<T>::st(o + j, v[j]);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void unpack_kernel(const T* __restrict__ in, int64_t ld, int B, int C, int64_t HW,
                                                          float* __restrict__ out) {
    GMD_WG_TRACE_SCOPE(WGK_UNPACK);
    const int64_t total = (int64_t)B * C * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t p = i % HW;
        const int64_t bc = i / HW;
        const int64_t b = bc / C, c = bc - b * C;
        out[i] = Elem<T>::ld(in + (b * HW + p) * ld + c);
    }
}

// img2img start / inpaint blend of one step, in the float32 operation order of the torch expressions (no FMA contraction):
//   keep   = noise ? ca * z0 + cb * noise : z0           scheduler.add_noise(z0, noise, t_next); z0 itself at the last step
//   x_prev = mask ? (1 - m) * keep + m * x_prev : keep   diffusers' inpaint rule; with a null mask x_prev is written, never read
//   x0     = (1 - m) * z0 + m * x0                       the clean picture where it is kept (x0 may be nullptr)
// mask: [mask_rows, hw], one row for every sample or one per sample, broadcast over the C channels.  No shortcut at m == 0 or 1:
// 0 * inf is NaN here as in torch.  x_prev and x0 are read and written by the same thread only.
__global__ __launch_bounds__(kThreads) void inpaint_blend_kernel(float* __restrict__ x_prev, float* __restrict__ x0,
                                                                 const float* __restrict__ mask, const float* __restrict__ z0,
                                                                 const float* __restrict__ noise, int64_t n, int64_t chw, int64_t hw,
                                                                 int per_sample, float ca, float cb) {
    GMD_WG_TRACE_SCOPE(WGK_LATENT_STEP);
    const unsigned threads = __builtin_amdgcn_workgroup_size_x();
    const int64_t stride = (int64_t)gridDim.x * threads;
    for (int64_t i = (int64_t)blockIdx.x * threads + threadIdx.x; i < n; i += stride) {
        const float z = z0[i];
        const float keep = noise ? ca * z + cb * noise[i] : z;
        if (!mask) {
            x_prev[i] = keep;
            continue;
        }
        const int64_t p = i % hw;
        const float m = mask[(per_sample ? (i / chw) * hw : 0) + p];
        const float om = 1.0f - m;
        if (x_prev) x_prev[i] = om * keep + m * x_prev[i];
        if (x0) x0[i] = om * z + m * x0[i];
    }
}

inline int grid_for(int64_t n) {
    int64_t g = (n + kThreads - 1) / kThreads;
    if (g > 2048) g = 2048;
    if (g < 1) g = 1;
    return (int)g;
}

// The launch tail of every gmd_*_step, after its own argument checks: the grid over B * chw elements, the rule that the rescale
// ratio counts only under CFG, the launch and its check.  `args`: what the kernel takes after its StepIn.
template <typename Kernel, typename... Args>
int launch_step(const char* name, Kernel kernel, gmd_stream_t stream, StepIn in, Args... args) {
    if (!in.do_cfg) in.ratio = nullptr;
    kernel<<<grid_for((int64_t)in.B * in.chw), kThreads, 0, (hipStream_t)stream>>>(in, args...);
    GMD_CHECK_LAUNCH(name);
    return GMD_OK;
}

}  // namespace

extern "C" {

int gmd_latent_step(const float* eps_in, const float* x, const float* cur_sample, const float* e1, const float* e2,
                    const float* e3, int B, int64_t chw, int do_cfg, float guidance_scale, const float* rescale_ratio,
                    float guidance_rescale, int mode, float sample_coeff, float alpha_delta, float denom,
                    float sqrt_alpha, float sqrt_one_minus_alpha, float* eps_out, float* x_prev, float* x0,
                    gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && chw >= 0, "gmd_latent_step: negative shape");
    GMD_REQUIRE(mode >= 0 && mode <= 4, "gmd_latent_step: mode %d not in 0..4", mode);
    if ((int64_t)B * chw == 0) return GMD_OK;
    GMD_REQUIRE(eps_in && x && x_prev, "gmd_latent_step: null pointer");
    GMD_REQUIRE(mode != 1 || (cur_sample && e1), "gmd_latent_step: mode 1 needs cur_sample and e1");
    GMD_REQUIRE(mode < 2 || e1, "gmd_latent_step: mode %d needs e1", mode);
    GMD_REQUIRE(mode < 3 || e2, "gmd_latent_step: mode %d needs e2", mode);
    GMD_REQUIRE(mode < 4 || e3, "gmd_latent_step: mode 4 needs e3");
    GMD_REQUIRE(denom != 0.0f && sqrt_alpha != 0.0f, "gmd_latent_step: zero denominator");
    return launch_step("gmd_latent_step", latent_step_kernel, stream,
                       StepIn{eps_in, x, B, chw, do_cfg, guidance_scale, rescale_ratio, guidance_rescale}, cur_sample, e1, e2, e3, mode,
                       sample_coeff, alpha_delta, denom, sqrt_alpha, sqrt_one_minus_alpha, eps_out, x_prev, x0);
}

int gmd_dpm_step(const float* eps_in, const float* x, const float* m1, int B, int64_t chw, int do_cfg, float guidance_scale,
                 const float* rescale_ratio, float guidance_rescale, int order, float sigma_s0, float alpha_s0, float c_x, float c_m,
                 float c_h, float inv_r0, float sqrt_alpha, float sqrt_one_minus_alpha, float* m0_out, float* x_prev, float* x0,
                 gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && chw > 0, "gmd_dpm_step: bad shape B=%d chw=%lld", B, (long long)chw);
    if (B == 0) return GMD_OK;
    GMD_REQUIRE(eps_in && x && m0_out && x_prev, "gmd_dpm_step: null pointer");
    GMD_REQUIRE(order == 1 || order == 2, "gmd_dpm_step: order must be 1 or 2 (got %d)", order);
    GMD_REQUIRE(order == 1 || m1, "gmd_dpm_step: the second-order update needs the previous x0 prediction");
    GMD_REQUIRE(alpha_s0 != 0.0f && (x0 == nullptr || sqrt_alpha != 0.0f), "gmd_dpm_step: zero denominator");
    return launch_step("gmd_dpm_step", dpm_step_kernel, stream,
                       StepIn{eps_in, x, B, chw, do_cfg, guidance_scale, rescale_ratio, guidance_rescale}, m1, order, sigma_s0, alpha_s0,
                       c_x, c_m, c_h, inv_r0, sqrt_alpha, sqrt_one_minus_alpha, m0_out, x_prev, x0);
}

int gmd_dpm_sde_step(const float* eps_in, const float* x, const float* m1, const float* noise, int B, int64_t chw, int do_cfg,
                     float guidance_scale, const float* rescale_ratio, float guidance_rescale, int order, float sigma_s0, float alpha_s0,
                     float c_x, float c_m, float c_h, float inv_r0, float c_n, float sqrt_alpha, float sqrt_one_minus_alpha,
                     float* m0_out, float* x_prev, float* x0, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && chw > 0, "gmd_dpm_sde_step: bad shape B=%d chw=%lld", B, (long long)chw);
    if (B == 0) return GMD_OK;
    GMD_REQUIRE(eps_in && x && m0_out && x_prev, "gmd_dpm_sde_step: null pointer");
    GMD_REQUIRE(noise, "gmd_dpm_sde_step: null noise pointer (the SDE update adds noise at every step)");
    GMD_REQUIRE(order == 1 || order == 2, "gmd_dpm_sde_step: order must be 1 or 2 (got %d)", order);
    GMD_REQUIRE(order == 1 || m1, "gmd_dpm_sde_step: the second-order update needs the previous x0 prediction");
    GMD_REQUIRE(alpha_s0 != 0.0f && (x0 == nullptr || sqrt_alpha != 0.0f), "gmd_dpm_sde_step: zero denominator");
    // written as !(v >= 0) so that a NaN (the square root of a negative 1 - exp(-2h)) is refused too
    GMD_REQUIRE(c_n >= 0.0f, "gmd_dpm_sde_step: c_n must be >= 0 (got %g)", (double)c_n);
    return launch_step("gmd_dpm_sde_step", dpm_sde_step_kernel, stream,
                       StepIn{eps_in, x, B, chw, do_cfg, guidance_scale, rescale_ratio, guidance_rescale}, m1, noise, order, sigma_s0,
                       alpha_s0, c_x, c_m, c_h, inv_r0, c_n, sqrt_alpha, sqrt_one_minus_alpha, m0_out, x_prev, x0);
}

int gmd_ddpm_step(const float* eps_in, const float* x, const float* noise, int B, int64_t chw, int do_cfg, float guidance_scale,
                  const float* rescale_ratio, float guidance_rescale, float sched_sqrt_alpha, float sched_sqrt_one_minus_alpha,
                  int clip_sample, float clip_range, float x0_coeff, float xt_coeff, float noise_scale, float sqrt_alpha,
                  float sqrt_one_minus_alpha, float* x_prev, float* x0, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && chw > 0, "gmd_ddpm_step: bad shape B=%d chw=%lld", B, (long long)chw);
    if (B == 0) return GMD_OK;
    GMD_REQUIRE(eps_in && x && x_prev, "gmd_ddpm_step: null pointer");
    GMD_REQUIRE(sched_sqrt_alpha != 0.0f && (x0 == nullptr || sqrt_alpha != 0.0f), "gmd_ddpm_step: zero denominator");
    GMD_REQUIRE(!clip_sample || clip_range > 0.0f, "gmd_ddpm_step: clip_range must be positive");
    return launch_step("gmd_ddpm_step", ddpm_step_kernel, stream,
                       StepIn{eps_in, x, B, chw, do_cfg, guidance_scale, rescale_ratio, guidance_rescale}, noise, sched_sqrt_alpha,
                       sched_sqrt_one_minus_alpha, clip_sample, clip_range, x0_coeff, xt_coeff, noise_scale, sqrt_alpha,
                       sqrt_one_minus_alpha, x_prev, x0);
}

int gmd_ddim_step(const float* eps_in, const float* x, const float* noise, int B, int64_t chw, int do_cfg, float guidance_scale,
                  const float* rescale_ratio, float guidance_rescale, float sched_sqrt_alpha, float sched_sqrt_one_minus_alpha,
                  int clip_sample, float clip_range, int use_clipped, float sqrt_alpha_prev, float dir_coeff, float std_dev,
                  float sqrt_alpha, float sqrt_one_minus_alpha, float* x_prev, float* x0, float* pred_x0, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && chw > 0, "gmd_ddim_step: bad shape B=%d chw=%lld", B, (long long)chw);
    if (B == 0) return GMD_OK;
    GMD_REQUIRE(eps_in && x && x_prev, "gmd_ddim_step: null pointer");
    GMD_REQUIRE(sched_sqrt_alpha != 0.0f && (!use_clipped || sched_sqrt_one_minus_alpha != 0.0f) &&
                    (x0 == nullptr || sqrt_alpha != 0.0f),
                "gmd_ddim_step: zero denominator");
    GMD_REQUIRE(!clip_sample || clip_range > 0.0f, "gmd_ddim_step: clip_range must be positive");
    // written as !(v >= 0) so that a NaN (the square root of a negative 1 - a_prev - std^2) is refused too
    GMD_REQUIRE(dir_coeff >= 0.0f, "gmd_ddim_step: dir_coeff must be >= 0 (got %g)", (double)dir_coeff);
    GMD_REQUIRE(std_dev >= 0.0f, "gmd_ddim_step: std_dev must be >= 0 (got %g)", (double)std_dev);
    return launch_step("gmd_ddim_step", ddim_step_kernel, stream,
                       StepIn{eps_in, x, B, chw, do_cfg, guidance_scale, rescale_ratio, guidance_rescale}, noise, sched_sqrt_alpha,
                       sched_sqrt_one_minus_alpha, clip_sample, clip_range, use_clipped, sqrt_alpha_prev, dir_coeff, std_dev,
                       sqrt_alpha, sqrt_one_minus_alpha, x_prev, x0, pred_x0);
}

int gmd_lcm_step(const float* eps_in, const float* x, const float* noise, int B, int64_t chw, int do_cfg, float guidance_scale,
                 const float* rescale_ratio, float guidance_rescale, float sched_sqrt_alpha, float sched_sqrt_one_minus_alpha,
                 int clip_sample, float clip_range, float c_skip, float c_out, float sqrt_alpha_prev, float sqrt_beta_prev,
                 float sqrt_alpha, float sqrt_one_minus_alpha, float* x_prev, float* x0, float* denoised, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && chw > 0, "gmd_lcm_step: bad shape B=%d chw=%lld", B, (long long)chw);
    // every scalar the kernel multiplies by: a NaN coefficient (a negative alpha under the square root) is refused before the launch
    const float c[6] = {sched_sqrt_alpha, sched_sqrt_one_minus_alpha, c_skip, c_out, sqrt_alpha_prev, sqrt_beta_prev};
    const char* const names[6] = {"sched_sqrt_alpha", "sched_sqrt_one_minus_alpha", "c_skip", "c_out", "sqrt_alpha_prev", "sqrt_beta_prev"};
    for (int k = 0; k < 6; ++k) GMD_REQUIRE(std::isfinite(c[k]), "gmd_lcm_step: %s must be finite (got %g)", names[k], (double)c[k]);
    GMD_REQUIRE(x0 == nullptr || (std::isfinite(sqrt_alpha) && std::isfinite(sqrt_one_minus_alpha)),
                "gmd_lcm_step: the pipeline x0 coefficients must be finite (got %g, %g)", (double)sqrt_alpha, (double)sqrt_one_minus_alpha);
    GMD_REQUIRE(sched_sqrt_alpha != 0.0f && (x0 == nullptr || sqrt_alpha != 0.0f), "gmd_lcm_step: zero denominator");
    GMD_REQUIRE(!clip_sample || clip_range > 0.0f, "gmd_lcm_step: clip_range must be positive");
    if (B == 0) return GMD_OK;
    GMD_REQUIRE(eps_in && x && x_prev, "gmd_lcm_step: null pointer");
    return launch_step("gmd_lcm_step", lcm_step_kernel, stream,
                       StepIn{eps_in, x, B, chw, do_cfg, guidance_scale, rescale_ratio, guidance_rescale}, noise, sched_sqrt_alpha,
                       sched_sqrt_one_minus_alpha, clip_sample, clip_range, c_skip, c_out, sqrt_alpha_prev, sqrt_beta_prev, sqrt_alpha,
                       sqrt_one_minus_alpha, x_prev, x0, denoised);
}

int gmd_euler_step(const float* eps_in, const float* x, const float* noise, int B, int64_t chw, int do_cfg, float guidance_scale,
                   const float* rescale_ratio, float guidance_rescale, float sigma_hat, float dt, float sigma_up, float* x_prev,
                   float* pred_x0, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && chw > 0, "gmd_euler_step: bad shape B=%d chw=%lld", B, (long long)chw);
    // written as (v > 0) / (v >= 0) so that a NaN is refused too
    GMD_REQUIRE(sigma_hat > 0.0f, "gmd_euler_step: sigma_hat must be > 0 (got %g)", (double)sigma_hat);
    GMD_REQUIRE(sigma_up >= 0.0f, "gmd_euler_step: sigma_up must be >= 0 (got %g)", (double)sigma_up);
    GMD_REQUIRE(std::isfinite(dt), "gmd_euler_step: dt must be finite (got %g)", (double)dt);
    if (B == 0) return GMD_OK;
    GMD_REQUIRE(eps_in && x && x_prev, "gmd_euler_step: null pointer");
    return launch_step("gmd_euler_step", euler_step_kernel, stream,
                       StepIn{eps_in, x, B, chw, do_cfg, guidance_scale, rescale_ratio, guidance_rescale}, noise, sigma_hat, dt, sigma_up,
                       x_prev, pred_x0);
}

int gmd_lms_step(const float* eps_in, const float* x, const float* d1, const float* d2, const float* d3, int B, int64_t chw, int do_cfg,
                 float guidance_scale, const float* rescale_ratio, float guidance_rescale, int order, float sigma, float c0, float c1,
                 float c2, float c3, float* d_out, float* x_prev, float* pred_x0, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && chw > 0, "gmd_lms_step: bad shape B=%d chw=%lld", B, (long long)chw);
    GMD_REQUIRE(order >= 1 && order <= 4, "gmd_lms_step: order %d not in 1..4", order);
    // written as (v > 0) so that a NaN is refused too
    GMD_REQUIRE(sigma > 0.0f, "gmd_lms_step: sigma must be > 0 (got %g)", (double)sigma);
    const float c[4] = {c0, c1, c2, c3};
    for (int k = 0; k < order; ++k)  // a coefficient beyond the order is never used
        GMD_REQUIRE(std::isfinite(c[k]), "gmd_lms_step: coefficient c%d must be finite (got %g)", k, (double)c[k]);
    if (B == 0) return GMD_OK;
    GMD_REQUIRE(eps_in && x && d_out && x_prev, "gmd_lms_step: null pointer");
    GMD_REQUIRE(order < 2 || d1, "gmd_lms_step: order %d needs d1", order);
    GMD_REQUIRE(order < 3 || d2, "gmd_lms_step: order %d needs d2", order);
    GMD_REQUIRE(order < 4 || d3, "gmd_lms_step: order 4 needs d3");
    return launch_step("gmd_lms_step", lms_step_kernel, stream,
                       StepIn{eps_in, x, B, chw, do_cfg, guidance_scale, rescale_ratio, guidance_rescale}, d1, d2, d3, order, sigma, c0,
                       c1, c2, c3, d_out, x_prev, pred_x0);
}

int gmd_unipc_step(const float* eps_in, const float* x, const float* last_sample, const float* h1, const float* h2, const float* h3, int B,
                   int64_t chw, int do_cfg, float guidance_scale, const float* rescale_ratio, float guidance_rescale, int corr_order,
                   int pred_order, float sigma_s, float alpha_s, float c_x, float c_m, float c_b, float c_rho1, float c_rho2, float c_rho3,
                   float c_r1, float c_r2, float p_x, float p_m, float p_b, float p_rho1, float p_rho2, float p_r1, float p_r2,
                   float sqrt_alpha, float sqrt_one_minus_alpha, float* m0_out, float* x_corr, float* x_prev, float* x0,
                   gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && chw > 0, "gmd_unipc_step: bad shape B=%d chw=%lld", B, (long long)chw);
    GMD_REQUIRE(corr_order >= 0 && corr_order <= 3, "gmd_unipc_step: corrector order %d not in 0..3", corr_order);
    GMD_REQUIRE(pred_order >= 1 && pred_order <= 3, "gmd_unipc_step: predictor order %d not in 1..3", pred_order);
    GMD_REQUIRE(std::isfinite(sigma_s), "gmd_unipc_step: sigma_s must be finite (got %g)", (double)sigma_s);
    GMD_REQUIRE(std::isfinite(alpha_s) && alpha_s != 0.0f, "gmd_unipc_step: alpha_s must be finite and non-zero (got %g)", (double)alpha_s);
    GMD_REQUIRE(x0 == nullptr || (std::isfinite(sqrt_alpha) && sqrt_alpha != 0.0f && std::isfinite(sqrt_one_minus_alpha)),
                "gmd_unipc_step: sqrt_alpha must be finite and non-zero, sqrt_one_minus_alpha finite, when x0 is asked for");
    // a scalar beyond the order is never used, so it is not looked at: at predictor order 1 that includes p_b (-inf at the last step of
    // a bh1 schedule that ends at sigma 0)
    if (corr_order >= 1) {
        const float c[3] = {c_x, c_m, c_b}, rho[3] = {c_rho1, c_rho2, c_rho3}, r[2] = {c_r1, c_r2};
        const char* names[3] = {"c_x", "c_m", "c_b"};
        for (int k = 0; k < 3; ++k) GMD_REQUIRE(std::isfinite(c[k]), "gmd_unipc_step: %s must be finite (got %g)", names[k], (double)c[k]);
        for (int k = 0; k < corr_order; ++k)
            GMD_REQUIRE(std::isfinite(rho[k]), "gmd_unipc_step: c_rho%d must be finite (got %g)", k + 1, (double)rho[k]);
        for (int k = 0; k < corr_order - 1; ++k)
            GMD_REQUIRE(std::isfinite(r[k]) && r[k] != 0.0f, "gmd_unipc_step: c_r%d must be finite and non-zero (got %g)", k + 1, (double)r[k]);
    }
    GMD_REQUIRE(std::isfinite(p_x), "gmd_unipc_step: p_x must be finite (got %g)", (double)p_x);
    GMD_REQUIRE(std::isfinite(p_m), "gmd_unipc_step: p_m must be finite (got %g)", (double)p_m);
    if (pred_order >= 2) {
        const float rho[2] = {p_rho1, p_rho2}, r[2] = {p_r1, p_r2};
        GMD_REQUIRE(std::isfinite(p_b), "gmd_unipc_step: p_b must be finite (got %g)", (double)p_b);
        for (int k = 0; k < pred_order - 1; ++k) {
            GMD_REQUIRE(std::isfinite(rho[k]), "gmd_unipc_step: p_rho%d must be finite (got %g)", k + 1, (double)rho[k]);
            GMD_REQUIRE(std::isfinite(r[k]) && r[k] != 0.0f, "gmd_unipc_step: p_r%d must be finite and non-zero (got %g)", k + 1, (double)r[k]);
        }
    }
    if (B == 0) return GMD_OK;
    GMD_REQUIRE(eps_in && x && m0_out && x_corr && x_prev, "gmd_unipc_step: null pointer");
    GMD_REQUIRE(corr_order < 1 || last_sample, "gmd_unipc_step: corrector order %d needs last_sample", corr_order);
    GMD_REQUIRE((corr_order < 1 && pred_order < 2) || h1, "gmd_unipc_step: corrector order %d / predictor order %d needs h1", corr_order, pred_order);
    GMD_REQUIRE((corr_order < 2 && pred_order < 3) || h2, "gmd_unipc_step: corrector order %d / predictor order %d needs h2", corr_order, pred_order);
    GMD_REQUIRE(corr_order < 3 || h3, "gmd_unipc_step: corrector order 3 needs h3");
    return launch_step("gmd_unipc_step", unipc_step_kernel, stream,
                       StepIn{eps_in, x, B, chw, do_cfg, guidance_scale, rescale_ratio, guidance_rescale}, last_sample, h1, h2, h3,
                       corr_order, pred_order, sigma_s, alpha_s, c_x, c_m, c_b, c_rho1, c_rho2, c_rho3, c_r1, c_r2, p_x, p_m, p_b, p_rho1,
                       p_rho2, p_r1, p_r2, sqrt_alpha, sqrt_one_minus_alpha, m0_out, x_corr, x_prev, x0);
}

int gmd_cfg_std_ratio(const float* eps_in, int B, int64_t chw, float guidance_scale, float* ratio, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && chw >= 2, "gmd_cfg_std_ratio: need at least 2 elements per sample");
    if (B == 0) return GMD_OK;
    GMD_REQUIRE(eps_in && ratio, "gmd_cfg_std_ratio: null pointer");
    cfg_std_ratio_kernel<<<B, kThreads, 0, (hipStream_t)stream>>>(eps_in, B, chw, guidance_scale, ratio);
    GMD_CHECK_LAUNCH("gmd_cfg_std_ratio");
    return GMD_OK;
}

int gmd_inpaint_blend(float* x_prev, float* x0, const float* mask, const float* z0, const float* noise, int B, int C, int64_t hw,
                      int mask_rows, float ca, float cb, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && C >= 0 && hw >= 0, "gmd_inpaint_blend: negative shape");
    GMD_REQUIRE(hw == 0 || (int64_t)B * C <= INT64_MAX / hw, "gmd_inpaint_blend: B * C * hw overflows");
    const int64_t n = (int64_t)B * C * hw;
    if (n == 0) return GMD_OK;
    GMD_REQUIRE(z0, "gmd_inpaint_blend: null z0");
    GMD_REQUIRE(x_prev || x0, "gmd_inpaint_blend: both outputs are null");
    GMD_REQUIRE(mask || !x0, "gmd_inpaint_blend: x0 is blended by the mask, which is null");
    GMD_REQUIRE(mask_rows == 1 || mask_rows == B, "gmd_inpaint_blend: mask_rows %d is neither 1 nor B = %d", mask_rows, B);
    inpaint_blend_kernel<<<grid_for(n), kThreads, 0, (hipStream_t)stream>>>(x_prev, x0, mask, z0, noise, n, (int64_t)C * hw, hw,
                                                                            mask_rows != 1, ca, cb);
    GMD_CHECK_LAUNCH("gmd_inpaint_blend");
    return GMD_OK;
}

int gmd_pack_unet_input(const float* src0, int C0, const float* src1, int C1, int B, int64_t HW, int dup, void* out,
                        int CP, int out_dtype, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && HW >= 0 && C0 > 0 && C1 >= 0, "gmd_pack_unet_input: bad shape");
    GMD_REQUIRE(CP % 8 == 0 && CP >= C0 + C1, "gmd_pack_unet_input: CP=%d must be a multiple of 8 and >= %d", CP, C0 + C1);
    GMD_REQUIRE(dup == 1 || dup == 2, "gmd_pack_unet_input: dup must be 1 or 2");
    GMD_REQUIRE(C1 == 0 || src1, "gmd_pack_unet_input: src1 is null");
    if ((int64_t)B * HW == 0) return GMD_OK;
    GMD_REQUIRE(src0 && out, "gmd_pack_unet_input: null pointer");
    const int64_t total = (int64_t)B * HW * (CP / 8);
    GMD_REQUIRE(gmd_known_dtype(out_dtype), "gmd_pack_unet_input: bad dtype %d", out_dtype);
    gmd_for_dtype(out_dtype, [&](auto tag) {
        using T = decltype(tag);
        pack_kernel<T, false><<<grid_for(total), kThreads, 0, (hipStream_t)stream>>>(src0, C0, 1.0f, src1, C1, 1.0f, B, HW, dup, (T*)out, CP);
    });
    GMD_CHECK_LAUNCH("gmd_pack_unet_input");
    return GMD_OK;
}

int gmd_pack_unet_input_scaled(const float* src0, int C0, float div0, const float* src1, int C1, float div1, int B, int64_t HW, int dup,
                               void* out, int CP, int out_dtype, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && HW >= 0 && C0 > 0 && C1 >= 0, "gmd_pack_unet_input_scaled: bad shape");
    GMD_REQUIRE(CP % 8 == 0 && CP >= C0 + C1, "gmd_pack_unet_input_scaled: CP=%d must be a multiple of 8 and >= %d", CP, C0 + C1);
    GMD_REQUIRE(dup == 1 || dup == 2, "gmd_pack_unet_input_scaled: dup must be 1 or 2");
    GMD_REQUIRE(C1 == 0 || src1, "gmd_pack_unet_input_scaled: src1 is null");
    // written as (v > 0) so that a NaN is refused too
    GMD_REQUIRE(div0 > 0.0f, "gmd_pack_unet_input_scaled: div0 must be > 0 (got %g)", (double)div0);
    GMD_REQUIRE(C1 == 0 || div1 > 0.0f, "gmd_pack_unet_input_scaled: div1 must be > 0 (got %g)", (double)div1);
    if ((int64_t)B * HW == 0) return GMD_OK;
    GMD_REQUIRE(src0 && out, "gmd_pack_unet_input_scaled: null pointer");
    const int64_t total = (int64_t)B * HW * (CP / 8);
    GMD_REQUIRE(gmd_known_dtype(out_dtype), "gmd_pack_unet_input_scaled: bad dtype %d", out_dtype);
    gmd_for_dtype(out_dtype, [&](auto tag) {
        using T = decltype(tag);
        pack_kernel<T, true><<<grid_for(total), kThreads, 0, (hipStream_t)stream>>>(src0, C0, div0, src1, C1, div1, B, HW, dup, (T*)out, CP);
    });
    GMD_CHECK_LAUNCH("gmd_pack_unet_input_scaled");
    return GMD_OK;
}

int gmd_unpack_nchw(const void* in, int in_dtype, int64_t ld, int B, int C, int64_t HW, float* out, gmd_stream_t stream) {
    GMD_REQUIRE(B >= 0 && C > 0 && HW >= 0 && ld >= C, "gmd_unpack_nchw: bad shape");
    if ((int64_t)B * HW == 0) return GMD_OK;
    GMD_REQUIRE(in && out, "gmd_unpack_nchw: null pointer");
    const int64_t total = (int64_t)B * C * HW;
    GMD_REQUIRE(gmd_known_dtype(in_dtype), "gmd_unpack_nchw: bad dtype %d", in_dtype);
    gmd_for_dtype(in_dtype, [&](auto tag) {
        using T = decltype(tag);
        unpack_kernel<T><<<grid_for(total), kThreads, 0, (hipStream_t)stream>>>((const T*)in, ld, B, C, HW, out);
    });
    GMD_CHECK_LAUNCH("gmd_unpack_nchw");
    return GMD_OK;
}

}  // extern "C"

GMD_WG_TRACE_SETTER(latent_step)
