// Resampling kernels of the full-resolution tail: the model runs at a working size, the product is written at the source picture's.
//   gmd_hdr_tail_resized  the fused tail (hdr_tail.hip) with each operand bilinearly resampled to an output size of its own
//   gmd_prepare_sdr       uint8 picture -> antialiased resize -> ToTensor -> Normalize: the VAE encoder's input
// HBM- / cache-bound gathers, no LDS.  Tap indices and weights come from exact INTEGER numerators and denominators: a float32 source
// coordinate alone costs ~5e-6 at 64 -> 240 (torch's own float32 F.interpolate shows it), several times the four-tap sum's error.
//
// Like hdr_tail.hip this file is built with -ffp-contract=off: the expressions below are evaluated as written.
#include "gmd_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int kThreads = 256;
constexpr int kMaxSide = 16384;  // every size of both entry points: numerators stay below 2^30 (see gmd_hip.h)

__device__ __forceinline__ float clamp01(float v) { return fminf(fmaxf(v, 0.0f), 1.0f); }

// the element arithmetic of hdr_tail.hip (eq1, u8_trunc, u16_code, rgbe_kernel), expression for expression
__device__ __forceinline__ float eq1(float sdr, float gm, float qmax, float eps, bool clamp_out) {
    float lin = powf(clamp01(sdr), 2.2f);
    float hdr = (lin + eps) * (1.0f + gm * qmax) - eps;
    if (clamp_out) hdr = fminf(fmaxf(hdr, 0.0f), qmax + 1.0f);
    return hdr;
}
__device__ __forceinline__ uint8_t u8_trunc(float x01) { return (uint8_t)(int)(x01 * 255.0f); }
__device__ __forceinline__ float u16_code(float x) { return rintf(fminf(fmaxf(x * 65535.0f, 0.0f), 65535.0f)); }
__device__ __forceinline__ uchar4 rgbe_px(float r, float g, float b) {
    r = fmaxf(r, 0.f); g = fmaxf(g, 0.f); b = fmaxf(b, 0.f);
    const float v = fmaxf(r, fmaxf(g, b));
    uchar4 px = make_uchar4(0, 0, 0, 0);
    if (v >= 1e-32f) {
        int e;
        const float m = frexpf(v, &e);
        const float sc = m * 256.0f / v;
        px = make_uchar4((uint8_t)(int)(r * sc), (uint8_t)(int)(g * sc), (uint8_t)(int)(b * sc), (uint8_t)(e + 128));
    }
    return px;
}

// Bilinear taps of output index i on an axis n_in -> n_out, half-pixel centres, edge clamp (cv2.INTER_LINEAR on float32 /
// F.interpolate(mode="bilinear", align_corners=False)): source coordinate ((2i+1) n_in - n_out) / (2 n_out), clamped at 0.
// lam's numerator is below den <= 2^15: both conversions are exact, lam carries the division's one rounding.
struct LinTap {
    int i0, i1;
    float lam;
};
__device__ __forceinline__ LinTap lin_tap(int i, int n_in, int n_out) {
    const int num = max((2 * i + 1) * n_in - n_out, 0), den = 2 * n_out;
    LinTap t;
    t.i0 = num / den;
    t.lam = (float)(num - t.i0 * den) / (float)den;
    t.i1 = min(t.i0 + 1, n_in - 1);
    return t;
}

// in_layout as in hdr_tail.hip: 0 planar [B,3,hw]; 1 interleaved [B,hw,3]; 2 interleaved [B,hw,4] (4th channel ignored)
template <typename T>
__device__ __forceinline__ float load_c(const T* base, int layout, int64_t b, int64_t p, int64_t hw, int c) {
    if (layout == 0) return Elem<T>::ld(base + (b * 3 + c) * hw + p);
    return Elem<T>::ld(base + (b * hw + p) * (layout == 1 ? 3 : 4) + c);
}

// clamp01(x/2 + 0.5) of each of the four taps (the scripts resize the post-processed image), then
// (1-ly)((1-lx) p00 + lx p01) + ly ((1-lx) p10 + lx p11).  With lam = 0 on both axes this is p00 itself, bit for bit.
template <typename T>
__device__ __forceinline__ void resample_px(const T* base, int layout, int64_t b, int h, int w, const LinTap& ty, const LinTap& tx, float (&v)[3]) {
    const int64_t hw = (int64_t)h * w;
    const int64_t p00 = (int64_t)ty.i0 * w + tx.i0, p01 = (int64_t)ty.i0 * w + tx.i1;
    const int64_t p10 = (int64_t)ty.i1 * w + tx.i0, p11 = (int64_t)ty.i1 * w + tx.i1;
    const float lx = tx.lam, ly = ty.lam;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float a00 = clamp01(load_c(base, layout, b, p00, hw, c) / 2.0f + 0.5f);
        const float a01 = clamp01(load_c(base, layout, b, p01, hw, c) / 2.0f + 0.5f);
        const float a10 = clamp01(load_c(base, layout, b, p10, hw, c) / 2.0f + 0.5f);
        const float a11 = clamp01(load_c(base, layout, b, p11, hw, c) / 2.0f + 0.5f);
        v[c] = (1.0f - ly) * ((1.0f - lx) * a00 + lx * a01) + ly * ((1.0f - lx) * a10 + lx * a11);
    }
}

// One output pixel per thread.  SRC_U8: the SDR operand is a uint8 [B,H,W,3] picture already at the output size, read as
// float(u8) / 255.0f (ToTensor); the gain map is resampled onto it.
template <typename T, bool SRC_U8>
__global__ __launch_bounds__(kThreads) void hdr_tail_resized_kernel(
    const void* __restrict__ sdr_in, int hs, int ws, const T* __restrict__ gm_dec, int hg, int wg, int layout, int B, int H, int W,
    float qmax, float eps, int flags, float* __restrict__ sdr_img, float* __restrict__ gm_img, uint8_t* __restrict__ sdr_u8,
    uint8_t* __restrict__ gm_u8, float* __restrict__ hdr, float* __restrict__ hdr_file, uint16_t* __restrict__ hdr_u16,
    uint8_t* __restrict__ hdr_rgbe) {
    const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
    const float qp1 = qmax + 1.0f;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / HW, p = i - b * HW;
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        float s[3], g[3], hf[3];
        if (SRC_U8) {
            const uint8_t* src = (const uint8_t*)sdr_in + i * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) s[c] = (float)src[c] / 255.0f;
        } else {
            resample_px((const T*)sdr_in, layout, b, hs, ws, lin_tap(y, hs, H), lin_tap(x, ws, W), s);
        }
        resample_px(gm_dec, layout, b, hg, wg, lin_tap(y, hg, H), lin_tap(x, wg, W), g);
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float sv = s[c], gv = g[c];
            const int64_t o = i * 3 + c;
            if (sdr_img) sdr_img[o] = sv;
            if (gm_img) gm_img[o] = gv;
            if (sdr_u8) sdr_u8[o] = u8_trunc(sv);
            if (gm_u8) gm_u8[o] = u8_trunc(gv);
            const float h = eq1(sv, gv, qmax, eps, flags & 1);
            if (hdr) hdr[o] = h;
            hf[c] = h / qp1;  // generate_hdr.py:28
            if (hdr_file) hdr_file[o] = hf[c];
            if (hdr_u16) hdr_u16[o] = (uint16_t)u16_code(hf[c]);
        }
        if (hdr_rgbe) *reinterpret_cast<uchar4*>(hdr_rgbe + i * 4) = rgbe_px(hf[0], hf[1], hf[2]);
    }
}

// ---- antialiased triangle filter (PIL's Image.resize(BILINEAR) / F.interpolate(mode="bilinear", antialias=True)) ----
// Taps of output index i on an axis n_in -> n_out as INTEGER weight numerators.  n_in >= n_out: tap j weighs
// max(0, 2 n_in - |(2j+1) n_out - (2i+1) n_in|), non-zero only for (2i-1) n_in < (2j+1) n_out < (2i+3) n_in: j runs over
// [lo / (2 n_out), hi / (2 n_out)] clipped to the picture (at most one zero-weight tap at either end).  n_in < n_out: the two
// bilinear taps of lin_tap with numerators den - r and r (a clamped edge names the same pixel twice).
struct AaAxis {
    int j0, count, n_in, n_out, i;
    bool down;
    int up_j0, up_j1, up_w0, up_w1;
    __device__ __forceinline__ void init(int i_, int n_in_, int n_out_) {
        i = i_; n_in = n_in_; n_out = n_out_;
        down = n_in >= n_out;
        if (down) {
            const int lo = max((2 * i - 1) * n_in, 0), hi = (2 * i + 3) * n_in;
            j0 = lo / (2 * n_out);
            count = min(n_in - 1, hi / (2 * n_out)) - j0 + 1;
        } else {
            const int num = max((2 * i + 1) * n_in - n_out, 0), den = 2 * n_out;
            const int i0 = num / den, r = num - i0 * den;
            up_j0 = i0; up_j1 = min(i0 + 1, n_in - 1);
            up_w0 = den - r; up_w1 = r;
            j0 = i0; count = 2;
        }
    }
    __device__ __forceinline__ int index(int k) const { return down ? j0 + k : (k == 0 ? up_j0 : up_j1); }
    __device__ __forceinline__ int weight(int k) const {
        if (!down) return k == 0 ? up_w0 : up_w1;
        return max(0, 2 * n_in - abs((2 * (j0 + k) + 1) * n_out - (2 * i + 1) * n_in));
    }
    __device__ __forceinline__ int sum() const {
        int s = 0;
        for (int k = 0; k < count; ++k) s += weight(k);
        return s;
    }
};

// One output pixel per thread, rows outer.  A row's sum_j nx_j * code_j is a sum of integers in float32 (exact below 2^24), divided
// once by the integer weight sum; the column pass repeats that over the row values; then ToTensor (/255), Normalize ((v-0.5)/0.5)
// and ONE rounding to T.  Equal sizes: one tap of weight 2n over a sum of 2n on both axes -- the code itself, so the result is
// ToTensor + Normalize exactly.  out_layout 0: [B,3,H,W]; 1: [B,H*W,cp] with channels 3..cp-1 zeroed (the encoder's padded input).
template <typename T>
__global__ __launch_bounds__(kThreads) void prepare_sdr_kernel(const uint8_t* __restrict__ src, int B, int h, int w, T* __restrict__ out,
                                                               int out_layout, int cp, int H, int W) {
    const int64_t HW = (int64_t)H * W, total = (int64_t)B * HW;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = i / HW, p = i - b * HW;
        const int y = (int)(p / W), x = (int)(p - (int64_t)y * W);
        AaAxis ay, ax;
        ay.init(y, h, H);
        ax.init(x, w, W);
        const float sx = (float)ax.sum(), sy = (float)ay.sum();
        const uint8_t* img = src + b * (int64_t)h * w * 3;
        float acc[3] = {0.0f, 0.0f, 0.0f};
        for (int ky = 0; ky < ay.count; ++ky) {
            const int wy = ay.weight(ky);
            if (wy == 0) continue;
            const uint8_t* row = img + (int64_t)ay.index(ky) * w * 3;
            float r[3] = {0.0f, 0.0f, 0.0f};
            for (int kx = 0; kx < ax.count; ++kx) {
                const float wx = (float)ax.weight(kx);
                const uint8_t* px = row + (int64_t)ax.index(kx) * 3;
#pragma unroll
                for (int c = 0; c < 3; ++c) r[c] = r[c] + wx * (float)px[c];
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = acc[c] + (float)wy * (r[c] / sx);
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v = (acc[c] / sy) / 255.0f;  // ToTensor
            const float o = (v - 0.5f) / 0.5f;       // Normalize([0.5], [0.5])
            if (out_layout == 0) Elem<T>::st(out + (b * 3 + c) * HW + p, o);
            else Elem<T>::st(out + i * cp + c, o);
        }
        if (out_layout != 0)
            for (int c = 3; c < cp; ++c) Elem<T>::st(out + i * cp + c, 0.0f);
    }
}

inline int grid_for(int64_t n) {
    int64_t g = (n + kThreads - 1) / kThreads;
    if (g > 256 * 32) g = 256 * 32;
    if (g < 1) g = 1;
    return (int)g;
}

inline bool aligned(const void* p, int a) { return p == nullptr || (reinterpret_cast<uintptr_t>(p) % a) == 0; }
inline bool side_ok(int n) { return n >= 1 && n <= kMaxSide; }

}  // namespace

extern "C" {

int gmd_hdr_tail_resized(const void* sdr, int hs, int ws, const void* gm_dec, int hg, int wg, int in_dtype, int in_layout, int B,
                         int H, int W, float qmax, float eps, int flags, float* sdr_img, float* gm_img, uint8_t* sdr_u8,
                         uint8_t* gm_u8, float* hdr, float* hdr_file, uint16_t* hdr_u16, uint8_t* hdr_rgbe, gmd_stream_t stream) {
    GMD_REQUIRE(sdr && gm_dec, "gmd_hdr_tail_resized: null input");
    GMD_REQUIRE(B >= 1, "gmd_hdr_tail_resized: B=%d must be positive", B);
    GMD_REQUIRE(side_ok(hs) && side_ok(ws) && side_ok(hg) && side_ok(wg) && side_ok(H) && side_ok(W),
                "gmd_hdr_tail_resized: every size must be in 1..%d (sdr %dx%d, gm %dx%d, out %dx%d)", kMaxSide, hs, ws, hg, wg, H, W);
    GMD_REQUIRE((int64_t)B * H * W * 4 <= INT64_C(0x7fffffffffff), "gmd_hdr_tail_resized: output too large");
    GMD_REQUIRE((flags & ~3) == 0, "gmd_hdr_tail_resized: flags %d: only bit 0 (clamp) and bit 1 (uint8 source) exist", flags);
    GMD_REQUIRE(in_layout >= 0 && in_layout <= 2, "gmd_hdr_tail_resized: in_layout must be 0 (NCHW), 1 (NHWC3) or 2 (NHWC4)");
    GMD_REQUIRE(gmd_known_dtype(in_dtype), "gmd_hdr_tail_resized: bad dtype %d", in_dtype);
    const bool src_u8 = (flags & 2) != 0;
    GMD_REQUIRE(!src_u8 || (hs == H && ws == W), "gmd_hdr_tail_resized: a uint8 source must already have the output size %dx%d, not %dx%d", H,
                W, hs, ws);
    const int esz = in_dtype == GMD_F32 ? 4 : 2;
    GMD_REQUIRE(aligned(gm_dec, esz) && aligned(sdr, src_u8 ? 1 : esz), "gmd_hdr_tail_resized: unaligned input");
    GMD_REQUIRE(aligned(sdr_img, 4) && aligned(gm_img, 4) && aligned(hdr, 4) && aligned(hdr_file, 4) && aligned(hdr_u16, 2) && aligned(hdr_rgbe, 4),
                "gmd_hdr_tail_resized: unaligned output");
    hipStream_t s = (hipStream_t)stream;
    const int grid = grid_for((int64_t)B * H * W);
    gmd_for_dtype(in_dtype, [&](auto tag) {
        using T = decltype(tag);
        if (src_u8)
            hdr_tail_resized_kernel<T, true><<<grid, kThreads, 0, s>>>(sdr, hs, ws, (const T*)gm_dec, hg, wg, in_layout, B, H, W, qmax, eps, flags,
                                                                      sdr_img, gm_img, sdr_u8, gm_u8, hdr, hdr_file, hdr_u16, hdr_rgbe);
        else
            hdr_tail_resized_kernel<T, false><<<grid, kThreads, 0, s>>>(sdr, hs, ws, (const T*)gm_dec, hg, wg, in_layout, B, H, W, qmax, eps, flags,
                                                                       sdr_img, gm_img, sdr_u8, gm_u8, hdr, hdr_file, hdr_u16, hdr_rgbe);
    });
    GMD_CHECK_LAUNCH("gmd_hdr_tail_resized");
    return GMD_OK;
}

int gmd_prepare_sdr(const uint8_t* src, int B, int h, int w, void* out, int out_dtype, int out_layout, int cp, int H, int W,
                    gmd_stream_t stream) {
    GMD_REQUIRE(src && out, "gmd_prepare_sdr: null pointer");
    GMD_REQUIRE(B >= 1, "gmd_prepare_sdr: B=%d must be positive", B);
    GMD_REQUIRE(side_ok(h) && side_ok(w) && side_ok(H) && side_ok(W), "gmd_prepare_sdr: every size must be in 1..%d (in %dx%d, out %dx%d)",
                kMaxSide, h, w, H, W);
    GMD_REQUIRE(out_layout == 0 || out_layout == 1, "gmd_prepare_sdr: out_layout must be 0 (NCHW) or 1 (channels-last, cp channels)");
    GMD_REQUIRE(out_layout == 0 || (cp >= 3 && cp <= 64), "gmd_prepare_sdr: cp=%d must be in 3..64", cp);
    GMD_REQUIRE(gmd_known_dtype(out_dtype), "gmd_prepare_sdr: bad dtype %d", out_dtype);
    GMD_REQUIRE(aligned(out, out_dtype == GMD_F32 ? 4 : 2), "gmd_prepare_sdr: unaligned output");
    gmd_for_dtype(out_dtype, [&](auto tag) {
        using T = decltype(tag);
        prepare_sdr_kernel<T><<<grid_for((int64_t)B * H * W), kThreads, 0, (hipStream_t)stream>>>(src, B, h, w, (T*)out, out_layout, cp, H, W);
    });
    GMD_CHECK_LAUNCH("gmd_prepare_sdr");
    return GMD_OK;
}

}  // extern "C"
