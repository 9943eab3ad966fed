// Pieces shared by the dense-contraction translation units (gemm.hip: 16-bit and exact float32 kernels; gemm_split.hip:
// float32 on the matrix cores as three float16 products): parameter block, operand addressing, LDS image, activation.
#pragma once
#include "gmd_common.h"
#include "gemm_params.h"
#include "gemm_plan.h"
#include <mutex>

using namespace gmd;  // GemmParams, Plan and the planner (gemm_params.h, gemm_plan.h)

// gemm_split.hip: float32 on the matrix cores as three float16 products (GMD_F32S / GMD_F32SW / GMD_F32SA), called by gmd_gemm_nt /
// gmd_gemm_qkv_vt / gmd_conv3x3 of gemm.hip, which validate the parameter block
// presplit: 0 = both operands plain float32 (GMD_F32S), 1 = W pre-split (GMD_F32SW), 2 = A and W pre-split (GMD_F32SA)
int gmd_launch_split_gemm(const GemmParams& p, int presplit, int batch, void* ws, int64_t ws_bytes, hipStream_t s, const char* name);
int gmd_launch_split_conv(const GemmParams& p, int presplit, void* ws, int64_t ws_bytes, hipStream_t s, const char* name);

namespace {

// (row tile, column tile) of linear tile index L under GemmParams::tile_group
__device__ __forceinline__ void grouped_tile(int L, int tiles_m, int tiles_n, int group, int& mt, int& nt) {
    if (group <= 1) {
        mt = L / tiles_n;
        nt = L - mt * tiles_n;
        return;
    }
    const int gsz = group * tiles_n;
    const int pg = L / gsz, r = L - pg * gsz;
    const int left = tiles_m - pg * group;
    const int rows = left < group ? left : group;  // the last group may be short
    nt = r / rows;
    mt = pg * group + (r - nt * rows);
}

// Row-invariant part of the A address of one staging slot.
struct RowCtx {
    bool valid;
    int b, oy, ox;         // conv: output pixel
    int64_t base;          // gemm: element offset of the row start
};

template <bool CONV>
__device__ __forceinline__ RowCtx make_row(const GemmParams& p, int m) {
    RowCtx r;
    r.valid = m < p.M;
    r.b = r.oy = r.ox = 0;
    r.base = 0;
    if (!r.valid) return r;
    if (CONV) {
        const int hw = p.Hout * p.Wout;
        r.b = m / hw;
        const int rem = m - r.b * hw;
        r.oy = rem / p.Wout;
        r.ox = rem - r.oy * p.Wout;
    } else {
        r.base = (int64_t)m * p.lda;
    }
    return r;
}

// element offset into A of (row, k-step starting at channel c0 of tap (ky,kx)), or -1 for padding
template <bool CONV>
__device__ __forceinline__ int64_t a_offset(const GemmParams& p, const RowCtx& r, int k0, int ky, int kx, int c0) {
    if (!r.valid) return -1;
    if (!CONV) return r.base + k0;
    int iy, ix;
    if (p.upsample) {
        const int uy = r.oy + ky - 1, ux = r.ox + kx - 1;
        if (uy < 0 || ux < 0 || uy >= p.Hout || ux >= p.Wout) return -1;  // Hout in {2 Hin - 1, 2 Hin} (host-checked): uy >> 1 < Hin
        iy = uy >> 1;
        ix = ux >> 1;
    } else {
        iy = r.oy * p.stride + ky - p.pad_lo;
        ix = r.ox * p.stride + kx - p.pad_lo;
        if (iy < 0 || ix < 0 || iy >= p.Hin || ix >= p.Win) return -1;
    }
    return (((int64_t)r.b * p.Hin + iy) * p.Win + ix) * p.Cin + c0;
}

// erf for the bf16 GEGLU epilogue: Abramowitz & Stegun 7.1.26, |error| <= 1.5e-7 (two orders below bf16 rounding) in ~14
// instructions (one v_rcp, one v_exp) instead of libm's branchy erff -- the epilogue of the K=320 ff1 GEMM evaluates 32 of
// them per thread for only 5 K steps of MFMA work.  The float32 parity path (gmd_geglu) keeps erff.
__device__ __forceinline__ float fast_erf(float x) {
    const float ax = fabsf(x);
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f, ax, 1.0f));
    float y = fmaf(1.061405429f, t, -1.453152027f);
    y = fmaf(y, t, 1.421413741f);
    y = fmaf(y, t, -0.284496736f);
    y = fmaf(y, t, 0.254829592f);
    y = y * t * __builtin_amdgcn_exp2f(-1.4426950408889634f * ax * ax);
    return copysignf(1.0f - y, x);
}

__device__ __forceinline__ float apply_act(float v, int act) {
    if (act == GMD_ACT_SILU) return silu_f(v);
    if (act == GMD_ACT_QUICK_GELU) return v / (1.0f + __expf(-1.702f * v));
    return v;
}

// ---- producer column statistics: the column pass of the row epilogues (gemm.hip epilogue_rows, gemm_split.hip epilogue_rows_f32) ----
// One float32 add that the compiler can neither pack with a neighbour nor fold away.  The column pass below keeps {sum, sum of
// squares} pairs; hipcc (ROCm 7.2) packs the pair updates into v_pk_add_f32 and, where the pair order of the two operands
// differs, adds `op_sel:[0,1] op_sel_hi:[1,0]`.  With the float32 kernels' register allocation that swizzled form sat two
// instructions in front of an EXEC change (the `column < NCOL` branch of the next 64 columns), and under a second stream's load
// lanes 48..63 of its low result came out without one of the two addends on three different MI355X (tools/stress_colstats.py:
// 1 launch in 200-1500).  Both halves of the pattern are gone: these adds are single v_add_f32, and the column
// loops run with every lane active (clamped column), only the stores predicated.
__device__ __forceinline__ float add_f32_single(float a, float b) {
    float r;
    asm volatile("v_add_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// cs[k] / cq[k] += column sums of the strip's 32 rows for column lane + 64 k (lanes past NCOL re-read the last column: never stored)
template <int NCOL, int ROWF>
__device__ __forceinline__ void colstats_pass(const float* strip, int lane, float (&cs)[(NCOL + 63) / 64], float (&cq)[(NCOL + 63) / 64]) {
#pragma unroll
    for (int k = 0; k < (NCOL + 63) / 64; ++k) {
        const int cc = lane + 64 * k < NCOL ? lane + 64 * k : NCOL - 1;
        float s_ = 0.f, q_ = 0.f;
#pragma unroll 8
        for (int r = 0; r < 32; ++r) {
            const float x = strip[r * ROWF + cc];
            s_ += x;
            q_ += x * x;
        }
        cs[k] = add_f32_single(cs[k], s_);
        cq[k] = add_f32_single(cq[k], q_);
    }
}

// {sum, sum of squares} of each bucket of `bucket` adjacent columns of this wave tile -> out[(row block) * (N / bucket) + ...]
template <int NCOL, int ROWF>
__device__ __forceinline__ void colstats_store(float* strip, int lane, const float (&cs)[(NCOL + 63) / 64], const float (&cq)[(NCOL + 63) / 64],
                                               int bucket, float* out) {
#pragma unroll
    for (int k = 0; k < (NCOL + 63) / 64; ++k) {
        const int cc = lane + 64 * k;
        if (cc < NCOL) {
            strip[cc] = cs[k];
            strip[ROWF + cc] = cq[k];
        }
    }
    __builtin_amdgcn_wave_barrier();
    const int nb = NCOL / bucket;
    const int b0 = (lane < nb ? lane : nb - 1) * bucket;  // every lane folds a bucket (the idle ones the last): no EXEC change around the adds
    float s_ = 0.f, q_ = 0.f;
    for (int e = 0; e < bucket; ++e) {
        s_ = add_f32_single(s_, strip[b0 + e]);
        q_ = add_f32_single(q_, strip[ROWF + b0 + e]);
    }
    if (lane < nb) *reinterpret_cast<float2*>(out + lane * 2) = make_float2(s_, q_);
}

// byte offset of 16-byte chunk `chunk` of row `row` in a [rows][128 B] tile; the XOR makes both the
// 8-lane ds_write_b128 groups and the 16-lane ds_read_b128 groups of a 16x16x32 fragment conflict-free
__device__ __forceinline__ int lds_off(int row, int chunk) { return row * 128 + ((chunk ^ ((row >> 1) & 7)) << 4); }

template <int V> struct IntC { static constexpr int value = V; };

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
constexpr unsigned kOOB = 0xFFFF0000u;  // byte offset beyond every buffer (extents are checked < kOOB on the host)

// Operand addressing of the bf16 kernel: every staging slot keeps ONE 32-bit byte offset into a raw buffer
// resource; rows beyond M/N and conv padding taps hold kOOB, for which the buffer load returns zeros -- no
// branches and no 64-bit arithmetic in the K loop.  For conv3x3 the offsets are recomputed only when the
// K loop crosses into the next filter tap (every Cin/64 steps).
template <bool CONV>
__device__ __forceinline__ unsigned conv_tap_offset(const GemmParams& p, bool valid, int b, int oy, int ox, int ky, int kx, int chunk) {
    if (!valid) return kOOB;
    int iy, ix;
    if (p.upsample) {
        const int uy = oy + ky - 1, ux = ox + kx - 1;
        if (uy < 0 || ux < 0 || uy >= p.Hout || ux >= p.Wout) return kOOB;  // Hout in {2 Hin - 1, 2 Hin} (host-checked): uy >> 1 < Hin
        iy = uy >> 1;
        ix = ux >> 1;
    } else {
        iy = oy * p.stride + ky - p.pad_lo;
        ix = ox * p.stride + kx - p.pad_lo;
        if (iy < 0 || ix < 0 || iy >= p.Hin || ix >= p.Win) return kOOB;
    }
    return (unsigned)(((b * p.Hin + iy) * p.Win + ix) * p.Cin) * 2u + (unsigned)chunk * 16u;
}

// Nearest-2x upsampling conv3x3 as four 2x2 phase convolutions (GemmParams::up2): tap (a, b) = (tap >> 1, tap & 1) of phase
// (py, px) = (ph >> 1, ph & 1) at low-resolution pixel (i, j) reads source pixel (i + a + py - 1, j + b + px - 1).  A virtual pixel
// outside [0, 2 Hin) is exactly a source pixel outside [0, Hin): the zero padding of the nine-tap form.
__device__ __forceinline__ unsigned up2_tap_offset(const GemmParams& p, bool valid, int b, int i, int j, int ph, int tap, int chunk) {
    if (!valid) return kOOB;
    const int iy = i + (tap >> 1) + (ph >> 1) - 1, ix = j + (tap & 1) + (ph & 1) - 1;
    if (iy < 0 || ix < 0 || iy >= p.Hin || ix >= p.Win) return kOOB;
    return (unsigned)(((b * p.Hin + iy) * p.Win + ix) * p.Cin) * 2u + (unsigned)chunk * 16u;
}

// ... and the output row of row r = (b, i, j) of phase ph: pixel (2 i + py, 2 j + px) of sample b (returned through `b`)
__device__ __forceinline__ int64_t up2_out_row(const GemmParams& p, int r, int ph, int& b) {
    const int hw = p.Hin * p.Win;
    b = r / hw;
    const int rem = r - b * hw;
    const int i = rem / p.Win, j = rem - i * p.Win;
    return ((int64_t)b * p.Hout + 2 * i + (ph >> 1)) * p.Wout + 2 * j + (ph & 1);
}

// The same map for the rows mw + ro, 0 <= ro < 64, of one wave tile, without a 32-bit division per row: (b0, i0, j0) of row mw is
// decoded once (mw is wave-uniform), and the two carries -- (j0 + ro) / Win and (i0 + carry) / Hin, dividends below 2^16 + 64 -- are
// float products corrected by one step either way (the rounded product is within 1 of the quotient for dividends below 2^22).
struct Up2Tile {
    int b0, i0, j0;
    float inv_w, inv_h;
};
__device__ __forceinline__ Up2Tile up2_tile(const GemmParams& p, int mw) {
    Up2Tile t;
    const int hw = p.Hin * p.Win;
    t.b0 = mw / hw;
    const int rem = mw - t.b0 * hw;
    t.i0 = rem / p.Win;
    t.j0 = rem - t.i0 * p.Win;
    t.inv_w = 1.0f / (float)p.Win;
    t.inv_h = 1.0f / (float)p.Hin;
    return t;
}
__device__ __forceinline__ int up2_small_div(int n, int d, float inv) {
    int q = (int)((float)n * inv);
    if (q * d > n) --q;
    if ((q + 1) * d <= n) ++q;
    return q;
}
__device__ __forceinline__ int64_t up2_tile_row(const GemmParams& p, const Up2Tile& t, int ro, int ph, int& b) {
    const int n = t.j0 + ro, cj = up2_small_div(n, p.Win, t.inv_w);
    const int j = n - cj * p.Win;
    const int n2 = t.i0 + cj, ci = up2_small_div(n2, p.Hin, t.inv_h);
    const int i = n2 - ci * p.Hin;
    b = t.b0 + ci;
    return ((int64_t)b * p.Hout + 2 * i + (ph >> 1)) * p.Wout + 2 * j + (ph & 1);
}

template <int N> __device__ __forceinline__ void wait_vmcnt() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory"); }

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is a per-(function, device) property: remember it per device, so a
// process that drives several GPUs (not the one-process-per-GPU design, but legal) opts in on each of them.
hipError_t opt_in_lds(const void* fn, int bytes) {
    constexpr int kMaxDev = 64, kMaxFn = 64;
    static const void* fns[kMaxFn];
    static unsigned long long done[kMaxFn];  // bit d: set on device d
    static std::mutex mu;
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    std::lock_guard<std::mutex> lock(mu);
    int slot = -1;
    for (int i = 0; i < kMaxFn; ++i) {
        if (fns[i] == fn) { slot = i; break; }
        if (fns[i] == nullptr) { fns[i] = fn; slot = i; break; }
    }
    if (slot >= 0 && dev < kMaxDev && (done[slot] >> dev & 1ull)) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (e == hipSuccess && slot >= 0 && dev < kMaxDev) done[slot] |= 1ull << dev;
    return e;
}

}  // namespace
