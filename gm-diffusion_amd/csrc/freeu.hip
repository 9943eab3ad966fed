// FreeU ("Free Lunch in Diffusion U-Net", diffusers' enable_freeu) on the HIP path: the skip concat of one FreeU site in ONE launch.
//
//   out[r, 0 : Ca/2]     = rnd(float(A[r, c]) * params[ib])                          the first half of the backbone channels
//   out[r, Ca/2 : Ca]    = A[r, c]
//   out[r, Ca : Ca + Cs] = rnd(float(S[r, c]) + (params[is] - 1) * low_{b,c}[y, x])    the Fourier-filtered skip;  r = (b H + y) W + x
//
// diffusers filters the skip as fftn -> fftshift -> mask -> ifftshift -> ifftn -> .real in float32, with threshold = 1: the mask is `scale`
// on the shifted bins [H/2 - 1, H/2] x [W/2 - 1, W/2], i.e. the frequencies {0, -1} x {0, -1} (an axis of length 1 holds {0} alone, an axis
// of length 2 both of its bins), and 1 elsewhere.  So the filter is X + (scale - 1) * low, low = the real part of the inverse transform of
// those at most four bins -- a seven-coefficient reduction per (sample, channel) and a rank-4 correction, no FFT:
//
//   c_uv = sum X[y, x] cos(u th_y + v ph_x),  d_uv = sum X[y, x] sin(u th_y + v ph_x),   th_y = 2 pi y / H, ph_x = 2 pi x / W
//   low[y, x] = 1 / (H W) * sum_{(u, v)} (c_uv cos(u th_y + v ph_x) + d_uv sin(u th_y + v ph_x)),   (u, v) in {0, 1}^2, u = 1 only if H > 1,
//                                                                                                  v = 1 only if W > 1
//
// (the bin set holds -1 without +1, so it is NOT conjugate-symmetric: a pure cos(th_y) comes out scaled by (1 + s) / 2 for H > 2.)
//
// A skip workgroup owns one sample and eight 16-byte vectors of channels (64 channels in 16 bits, 32 in float32); thread t holds vector
// t % 8 of the pixels t / 8, t / 8 + 32, ...  Pass 1: each thread adds its pixels' seven products serially, in pixel order; the 32 pixel
// lanes meet through LDS and are added serially, lane 0 first.  Pass 2: the SAME thread re-reads the SAME elements (cache resident: 8 -- 128
// KB per block at 8x8 ... 32x32), adds the correction and stores.  So the summation order depends on (H, W) alone -- a sample's result
// does not depend on what else is in the launch, no atomics -- and every element is read for the last time and written by one lane, after
// a barrier behind every read that feeds its channel's coefficients: `out` may be the buffer A and S are views of (in place, behind
// gmd_concat_channels_add).  The cos / sin of the H + W phases are tabulated once per workgroup in LDS, from sinpif / cospif of an argument
// reduced in the INTEGER index to [0, 1/2] (no rounded 2 pi y / H); the mixed bin is formed from products.  Further workgroups of the
// launch copy / scale the A part.  params[is] == 1 / params[ib] == 1: that part is a raw copy (bit-identical, no arithmetic).
//
// `params` lives in DEVICE memory and is read by the kernel (the convention of gmd_scaled_add / gmd_lora_update): one captured graph serves
// every setting.  Built with -ffp-contract=off (the Makefile's NOFMA list): the arithmetic is the one tests/freeu_ref.py restates.
#include "gmd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kVecCols = 8;                      // 16-byte vectors of one pixel a skip workgroup owns
constexpr int kPixLanes = kThreads / kVecCols;   // 32 pixel-strided lanes per vector column
constexpr int kSums = 7;                         // DC, and {cos, sin} of the bins (1, 0), (0, 1), (1, 1)
constexpr int kMaxBackboneGrid = 1024;           // workgroups of the A part (then grid-stride laps)
constexpr int kMaxLdsBytes = 64 * 1024;

// cos and sin of 2 pi i / n for 0 <= i < n, the argument reduced in integers: 2 pi i / n = pi * m / n with m = 2 i folded into [0, n / 2]
__device__ __forceinline__ void phase(int i, int n, float& c, float& s) {
    int m = 2 * i;               // angle = pi * m / n, m in [0, 2n)
    float sgn_s = 1.0f, sgn_c = 1.0f;
    if (m > n) { m = 2 * n - m; sgn_s = -1.0f; }          // cos(2 pi - a) = cos a, sin(2 pi - a) = -sin a;   m in [0, n]
    if (2 * m > n) { m = n - m; sgn_c = -1.0f; }          // cos(pi - a) = -cos a, sin(pi - a) = sin a;       m / n in [0, 1/2]
    const float a = (float)m / (float)n;
    c = sgn_c * cospif(a);
    s = sgn_s * sinpif(a);
}

template <typename T>
__global__ __launch_bounds__(kThreads) void concat_freeu_kernel(const T* A, int Ca, int64_t lda, const T* S, int Cs, int64_t lds, T* out,
                                                                int64_t ldo, int B, int H, int W, const float* __restrict__ params, int ib,
                                                                int is, int ncb, int nskip) {
#pragma clang fp contract(off)
    GMD_WG_TRACE_SCOPE(WGK_CONCAT);
    constexpr int V = Elem<T>::kVec;
    constexpr int CB = kVecCols * V;  // channels of a skip workgroup
    extern __shared__ float smem[];
    const int t = threadIdx.x;
    const int HW = H * W;

    if ((int)blockIdx.x >= nskip) {
        // ---- the backbone part: first half scaled, second half copied (nothing to do for it in place)
        const float b = params[ib];
        const int CaV = Ca / V, half = CaV / 2;
        const int64_t total = (int64_t)B * HW * CaV;
        const int nblk = (int)gridDim.x - nskip;
        for (int64_t i = (int64_t)((int)blockIdx.x - nskip) * kThreads + t; i < total; i += (int64_t)nblk * kThreads) {
            const int64_t r = i / CaV;
            const int c = (int)(i - r * CaV);
            const T* src = A + r * lda + (int64_t)c * V;
            T* dst = out + r * ldo + (int64_t)c * V;
            if (c >= half || b == 1.0f) {
                if (src != dst) *reinterpret_cast<uint4*>(dst) = *reinterpret_cast<const uint4*>(src);
                continue;
            }
            float x[V];
            load_vec(src, x);
#pragma unroll
            for (int j = 0; j < V; ++j) x[j] = __fmul_rn(x[j], b);
            store_vec(dst, x);  // the one rounding: torch's `h * b` on a tensor of T with a float32 scalar
        }
        return;
    }

    // ---- one sample, one block of skip channels
    const int b = (int)blockIdx.x / ncb, cb = (int)blockIdx.x - b * ncb;
    const int vc = t % kVecCols, pl = t / kVecCols;
    const int c0 = cb * CB + vc * V;
    const bool active = c0 < Cs;
    const T* src = S + (int64_t)b * HW * lds + c0;
    T* dst = out + (int64_t)b * HW * ldo + Ca + c0;
    const float s = params[is];
    if (s == 1.0f) {  // the filter is the identity: a raw copy (uniform over the launch)
        if (active && src != dst)
            for (int p = pl; p < HW; p += kPixLanes)
                *reinterpret_cast<uint4*>(dst + (int64_t)p * ldo) = *reinterpret_cast<const uint4*>(src + (int64_t)p * lds);
        return;
    }
    float* part = smem;                                  // [kPixLanes][kSums][CB]
    float* coef = part + kPixLanes * kSums * CB;         // [kSums][CB]
    float* cy = coef + kSums * CB;                       // cos th_y [H], sin th_y [H], cos ph_x [W], sin ph_x [W]
    float* sy = cy + H;
    float* cx = sy + H;
    float* sx = cx + W;
    for (int i = t; i < H; i += kThreads) phase(i, H, cy[i], sy[i]);
    for (int i = t; i < W; i += kThreads) phase(i, W, cx[i], sx[i]);
    __syncthreads();

    // pass 1: the seven sums of this thread's pixels, serially in pixel order
    float acc[kSums][V];
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) acc[k][j] = 0.0f;
    if (active) {
        for (int p = pl; p < HW; p += kPixLanes) {
            const int y = p / W, x = p - y * W;
            const float cyv = cy[y], syv = sy[y], cxv = cx[x], sxv = sx[x];
            const float c11 = cyv * cxv - syv * sxv, s11 = syv * cxv + cyv * sxv;  // cos / sin (th_y + ph_x)
            float v[V];
            load_vec(src + (int64_t)p * lds, v);
#pragma unroll
            for (int j = 0; j < V; ++j) {
                acc[0][j] += v[j];
                acc[1][j] += v[j] * cyv;
                acc[2][j] += v[j] * syv;
                acc[3][j] += v[j] * cxv;
                acc[4][j] += v[j] * sxv;
                acc[5][j] += v[j] * c11;
                acc[6][j] += v[j] * s11;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) part[(pl * kSums + k) * CB + vc * V + j] = acc[k][j];
    __syncthreads();  // every read of pass 1 is complete: from here on the block's elements may be overwritten
    for (int idx = t; idx < kSums * CB; idx += kThreads) {
        float a = 0.0f;
        for (int l = 0; l < kPixLanes; ++l) a += part[l * kSums * CB + idx];  // pixel lanes serially, lane 0 first
        coef[idx] = a;
    }
    __syncthreads();
    if (!active) return;

    // pass 2: the same thread, the same elements
    float cf[kSums][V];
#pragma unroll
    for (int k = 0; k < kSums; ++k)
#pragma unroll
        for (int j = 0; j < V; ++j) cf[k][j] = coef[k * CB + vc * V + j];
    const float g = (s - 1.0f) / (float)HW;
    const float gu = H > 1 ? g : 0.0f, gv = W > 1 ? g : 0.0f, guv = (H > 1 && W > 1) ? g : 0.0f;  // an axis of length 1 holds bin 0 alone
    for (int p = pl; p < HW; p += kPixLanes) {
        const int y = p / W, x = p - y * W;
        const float cyv = cy[y], syv = sy[y], cxv = cx[x], sxv = sx[x];
        const float c11 = cyv * cxv - syv * sxv, s11 = syv * cxv + cyv * sxv;
        const float w1 = gu * cyv, w2 = gu * syv, w3 = gv * cxv, w4 = gv * sxv, w5 = guv * c11, w6 = guv * s11;
        float v[V];
        load_vec(src + (int64_t)p * lds, v);
#pragma unroll
        for (int j = 0; j < V; ++j) {
            float d = g * cf[0][j];
            d += w1 * cf[1][j];
            d += w2 * cf[2][j];
            d += w3 * cf[3][j];
            d += w4 * cf[4][j];
            d += w5 * cf[5][j];
            d += w6 * cf[6][j];
            v[j] += d;
        }
        store_vec(dst + (int64_t)p * ldo, v);  // the one rounding
    }
}

inline bool ranges_overlap(const char* a0, const char* a1, const char* b0, const char* b1) { return a0 < b1 && b0 < a1; }

}  // namespace

extern "C" int gmd_concat_channels_freeu(const void* A, int Ca, int64_t lda, const void* S, int Cs, int64_t lds, void* out, int64_t ldo,
                                         int dtype, int B, int H, int W, const float* params, int ib, int is, gmd_stream_t stream) {
    GMD_REQUIRE(gmd_known_dtype(dtype), "gmd_concat_channels_freeu: bad dtype %d", dtype);
    GMD_REQUIRE(B >= 0 && Ca > 0 && Cs > 0, "gmd_concat_channels_freeu: bad shape B=%d Ca=%d Cs=%d", B, Ca, Cs);
    GMD_REQUIRE(H >= 1 && W >= 1, "gmd_concat_channels_freeu: H=%d and W=%d must be at least 1", H, W);
    const int cv = gmd_is_half(dtype) ? 8 : 4;
    const int es = gmd_is_half(dtype) ? 2 : 4;
    GMD_REQUIRE(Ca % (2 * cv) == 0 && Cs % cv == 0, "gmd_concat_channels_freeu: Ca / 2 and Cs must be multiples of %d", cv);
    GMD_REQUIRE(lda % cv == 0 && lds % cv == 0 && ldo % cv == 0, "gmd_concat_channels_freeu: the row strides must be multiples of %d", cv);
    GMD_REQUIRE(lda >= Ca && lds >= Cs && ldo >= (int64_t)Ca + Cs, "gmd_concat_channels_freeu: a row stride is smaller than its row");
    GMD_REQUIRE(params != nullptr, "gmd_concat_channels_freeu: params must be the float32 device array of the settings");
    GMD_REQUIRE(ib >= 0 && is >= 0, "gmd_concat_channels_freeu: negative index into params");
    if (B == 0) return GMD_OK;
    GMD_REQUIRE(A && S && out, "gmd_concat_channels_freeu: null pointer");
    GMD_REQUIRE(gmd_aligned16(A) && gmd_aligned16(S) && gmd_aligned16(out), "gmd_concat_channels_freeu: pointers must be 16-byte aligned");
    GMD_REQUIRE((int64_t)H * W < (1ll << 31) / B, "gmd_concat_channels_freeu: B * H * W beyond 2^31 - 1 rows");
    const int64_t rows = (int64_t)B * H * W;
    const int64_t abytes = ((rows - 1) * lda + Ca) * es, sbytes = ((rows - 1) * lds + Cs) * es, obytes = ((rows - 1) * ldo + Ca + Cs) * es;
    GMD_REQUIRE(abytes < (1ll << 31) && sbytes < (1ll << 31) && obytes < (1ll << 31),
                "gmd_concat_channels_freeu: a tensor exceeds 2 GiB (32-bit byte offsets)");
    const char *a0 = (const char*)A, *s0 = (const char*)S, *o0 = (const char*)out;
    const bool in_place = a0 == o0 && s0 == o0 + (int64_t)Ca * es && lda == ldo && lds == ldo;
    if (!in_place)
        GMD_REQUIRE(!ranges_overlap(a0, a0 + abytes, o0, o0 + obytes) && !ranges_overlap(s0, s0 + sbytes, o0, o0 + obytes) &&
                        !ranges_overlap(a0, a0 + abytes, s0, s0 + sbytes),
                    "gmd_concat_channels_freeu: A / S / out overlap (allowed only in place: A = out, S = out + Ca, one row stride)");
    const int cb = kVecCols * cv;
    const size_t smem = ((size_t)(kPixLanes + 1) * kSums * cb + 2 * ((size_t)H + W)) * sizeof(float);
    GMD_REQUIRE(smem <= (size_t)kMaxLdsBytes, "gmd_concat_channels_freeu: H + W = %lld beyond the phase tables (at most %d)",
                (long long)H + W, (int)((kMaxLdsBytes / sizeof(float) - (size_t)(kPixLanes + 1) * kSums * cb) / 2));
    const int ncb = (Cs + cb - 1) / cb;
    const int64_t nskip = (int64_t)B * ncb;
    int64_t na = (rows * (Ca / cv) + kThreads - 1) / kThreads;
    if (na > kMaxBackboneGrid) na = kMaxBackboneGrid;
    GMD_REQUIRE(nskip + na < (1ll << 31), "gmd_concat_channels_freeu: grid too large");
    gmd_for_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        concat_freeu_kernel<T><<<(int)(nskip + na), kThreads, smem, (hipStream_t)stream>>>((const T*)A, Ca, lda, (const T*)S, Cs, lds, (T*)out,
                                                                                          ldo, B, H, W, params, ib, is, ncb, (int)nskip);
    });
    GMD_CHECK_LAUNCH("gmd_concat_channels_freeu");
    return GMD_OK;
}

GMD_WG_TRACE_SETTER(freeu)
