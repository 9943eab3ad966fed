// ControlNet conditioning on the HIP path: the skip-connection concat with the ControlNet residuals added where the skip is read anyway
// (one more operand of the concat kernel, no extra pass over an activation), and the in-place SiLU of the conditioning embedding.
//
//   out[r, :Ca] = Ra ? rnd(A[r]  + rnd(Ra[r - r_row0] * scales[ia])) : A[r]
//   out[r, Ca:] = Rb ? rnd(Bm[r] + rnd(Rb[r - r_row0] * scales[ib])) : Bm[r]          (rows r < r_row0: plain copy)
//
// rnd = one rounding to the tensor's dtype; product and sum in float32, never contracted: bit for bit torch's `s + r * scale` on
// bf16 / f16 / float32 tensors with a float32 scalar.  (hipcc's __fmul_rn / __fadd_rn are a plain `*` / `+` and fuse under the default
// -ffp-contract=fast: the file is built with -ffp-contract=off, the Makefile's NOFMA list, and the expression sits under the pragma too.)  `scales` lives in DEVICE memory (13 floats: twelve down
// residuals and the mid residual) and is read by the kernel, so a captured graph serves every controlnet_conditioning_scale.
#include "gmd_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kScales = 13;       // residuals of an SD-1.5 ControlNet: 12 down + 1 mid
constexpr int kStatRows = 64;     // rows per statistics block (the format gmd_groupnorm_colstats reads)
constexpr int kMaxGrid = 2048;    // 8 workgroups of 256 threads per CU on 256 CUs: every lane of the chip, then grid-stride laps

template <typename T> __device__ __forceinline__ float round_to(float x);
template <> __device__ __forceinline__ float round_to<float>(float x) { return x; }
template <> __device__ __forceinline__ float round_to<bf16_t>(float x) { return Half<bf16_t>::round(x); }
template <> __device__ __forceinline__ float round_to<f16_t>(float x) { return Half<f16_t>::round(x); }

// one 16-byte vector i of the output (row r = i / CV): copy, or skip + scaled residual
template <typename T>
__device__ __forceinline__ void concat_add_vec(const T* __restrict__ A, int Ca, const T* __restrict__ Ra, float sa,
                                               const T* __restrict__ Bm, int Cb, const T* __restrict__ Rb, float sb, int64_t r_row0,
                                               T* out, int64_t i, int CV, int CaV) {
#pragma clang fp contract(off)
    constexpr int V = Elem<T>::kVec;
    const int64_t r = i / CV;
    const int c = (int)(i - r * CV);
    const bool in_a = c < CaV;
    const int C = in_a ? Ca : Cb;
    const int col = (in_a ? c : c - CaV) * V;
    const T* src = (in_a ? A : Bm) + r * C + col;
    const T* res = in_a ? Ra : Rb;
    if (res == nullptr || r < r_row0) {
        *reinterpret_cast<uint4*>(out + i * V) = *reinterpret_cast<const uint4*>(src);
        return;
    }
    const float s = in_a ? sa : sb;
    float x[V], q[V];
    load_vec(src, x);
    load_vec(res + (r - r_row0) * C + col, q);
#pragma unroll
    for (int j = 0; j < V; ++j) x[j] = __fadd_rn(x[j], round_to<T>(__fmul_rn(q[j], s)));
    store_vec(out + i * V, x);  // the one rounding of the sum
}

template <typename T>
__global__ __launch_bounds__(kThreads) void concat_add_kernel(const T* __restrict__ A, int Ca, const T* __restrict__ Ra, int ia,
                                                              const T* __restrict__ Bm, int Cb, const T* __restrict__ Rb, int ib,
                                                              const float* __restrict__ scales, int64_t r_row0, T* __restrict__ out,
                                                              int64_t rows) {
    GMD_WG_TRACE_SCOPE(WGK_CONCAT);
    constexpr int V = Elem<T>::kVec;
    const int CV = (Ca + Cb) / V, CaV = Ca / V;
    const float sa = Ra ? scales[ia] : 0.0f, sb = Rb ? scales[ib] : 0.0f;
    const int64_t total = rows * CV;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x)
        concat_add_vec<T>(A, Ca, Ra, sa, Bm, Cb, Rb, sb, r_row0, out, i, CV, CaV);
}

// The same stores, one workgroup per 64-row block, which then leaves {sum, sum of squares} of the STORED B-part values of its block per
// bucket of adjacent channels: stats[block][Cb / bucket][2], what a producer's row epilogue leaves for gmd_groupnorm_colstats.  Fixed
// order, no atomics: per column the 32 rows of each half block serially, the two halves, then the bucket's columns serially -- the
// addition chain of the producers (32 + 2 + bucket).  The block re-reads its own stores (64 x Cb elements, cache resident).
template <typename T>
__global__ __launch_bounds__(kThreads) void concat_add_stats_kernel(const T* __restrict__ A, int Ca, const T* __restrict__ Ra, int ia,
                                                                    const T* __restrict__ Bm, int Cb, const T* __restrict__ Rb, int ib,
                                                                    const float* __restrict__ scales, int64_t r_row0, T* out,
                                                                    float* __restrict__ stats, int bucket) {
    GMD_WG_TRACE_SCOPE(WGK_CONCAT);
    extern __shared__ float lds[];  // [2 halves][Cb] sums, then [2 halves][Cb] sums of squares
    constexpr int V = Elem<T>::kVec;
    const int C = Ca + Cb, CV = C / V, CaV = Ca / V;
    const float sa = Ra ? scales[ia] : 0.0f, sb = Rb ? scales[ib] : 0.0f;
    const int64_t row0 = (int64_t)blockIdx.x * kStatRows;
    const int64_t v0 = row0 * CV;
    for (int k = threadIdx.x; k < kStatRows * CV; k += kThreads)
        concat_add_vec<T>(A, Ca, Ra, sa, Bm, Cb, Rb, sb, r_row0, out, v0 + k, CV, CaV);
    __threadfence_block();
    __syncthreads();
    float* cs = lds;
    float* cq = lds + 2 * Cb;
    for (int w = threadIdx.x; w < 2 * Cb; w += kThreads) {
        const int half = w / Cb, c = w - half * Cb;
        const T* p = out + (row0 + half * 32) * C + Ca + c;
        float s = 0.0f, q = 0.0f;
        for (int r = 0; r < 32; ++r) {
            const float v = Elem<T>::ld(p + (int64_t)r * C);
            s = __fadd_rn(s, v);
            q = __fadd_rn(q, __fmul_rn(v, v));
        }
        cs[w] = s;
        cq[w] = q;
    }
    __syncthreads();
    const int nb = Cb / bucket;
    for (int b = threadIdx.x; b < nb; b += kThreads) {
        float s = 0.0f, q = 0.0f;
        for (int j = 0; j < bucket; ++j) {
            const int c = b * bucket + j;
            s = __fadd_rn(s, __fadd_rn(cs[c], cs[Cb + c]));
            q = __fadd_rn(q, __fadd_rn(cq[c], cq[Cb + c]));
        }
        float* o = stats + ((int64_t)blockIdx.x * nb + b) * 2;
        o[0] = s;
        o[1] = q;
    }
}

// x = x * sigmoid(x) in place, with the formula of the GroupNorm + SiLU kernels (silu_f of gmd_common.h: hardware reciprocal of
// 1 + __expf(-x)), float32 inside, one rounding on the store.  The conditioning embedding's seven activations: once per call.
template <typename T>
__global__ __launch_bounds__(kThreads) void silu_kernel(T* __restrict__ X, int64_t nvec) {
    GMD_WG_TRACE_SCOPE(WGK_OTHER);
    constexpr int V = Elem<T>::kVec;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nvec; i += (int64_t)gridDim.x * blockDim.x) {
        float v[V];
        load_vec(X + i * V, v);
#pragma unroll
        for (int j = 0; j < V; ++j) v[j] = silu_f(v[j]);
        store_vec(X + i * V, v);
    }
}

inline int grid_for(int64_t n) {
    int64_t g = (n + kThreads - 1) / kThreads;
    if (g > kMaxGrid) g = kMaxGrid;
    if (g < 1) g = 1;
    return (int)g;
}

}  // namespace

extern "C" {

int gmd_concat_channels_add(const void* A, int Ca, const void* Ra, int ia, const void* Bm, int Cb, const void* Rb, int ib,
                            const float* scales, int64_t r_row0, void* out, int dtype, int64_t rows, float* colstats_b,
                            int colstats_bucket, gmd_stream_t stream) {
    GMD_REQUIRE(rows >= 0 && Ca > 0 && Cb > 0, "gmd_concat_channels_add: bad shape");
    GMD_REQUIRE(r_row0 >= 0 && r_row0 <= rows, "gmd_concat_channels_add: r_row0=%lld outside [0, rows=%lld]", (long long)r_row0, (long long)rows);
    if (rows == 0) return GMD_OK;
    GMD_REQUIRE(A && Bm && out, "gmd_concat_channels_add: null pointer");
    GMD_REQUIRE(gmd_aligned16(A) && gmd_aligned16(Bm) && gmd_aligned16(out) && gmd_aligned16(Ra) && gmd_aligned16(Rb),
                "gmd_concat_channels_add: pointers must be 16-byte aligned");
    GMD_REQUIRE(gmd_known_dtype(dtype), "gmd_concat_channels_add: bad dtype %d", dtype);
    const int cv = gmd_is_half(dtype) ? 8 : 4;
    GMD_REQUIRE(Ca % cv == 0 && Cb % cv == 0, "gmd_concat_channels_add: channel counts must be multiples of %d", cv);
    if (Ra || Rb) {
        GMD_REQUIRE(scales != nullptr, "gmd_concat_channels_add: a residual needs the device array of scales");
        GMD_REQUIRE((!Ra || (ia >= 0 && ia < kScales)) && (!Rb || (ib >= 0 && ib < kScales)),
                    "gmd_concat_channels_add: scale index outside [0, %d)", kScales);
    }
    hipStream_t s = (hipStream_t)stream;
    if (colstats_b != nullptr) {
        GMD_REQUIRE(colstats_bucket > 0 && Cb % colstats_bucket == 0 && rows % kStatRows == 0,
                    "gmd_concat_channels_add: statistics need rows %% 64 == 0 and Cb %% bucket == 0");
        GMD_REQUIRE(rows / kStatRows <= 0x7fffffff && (int64_t)Cb * 16 <= 65536,
                    "gmd_concat_channels_add: statistics need Cb <= 4096 and at most 2^31 - 1 row blocks");
        const size_t lds = (size_t)Cb * 4 * sizeof(float);
        gmd_for_dtype(dtype, [&](auto tag) {
            using T = decltype(tag);
            concat_add_stats_kernel<T><<<(int)(rows / kStatRows), kThreads, lds, s>>>((const T*)A, Ca, (const T*)Ra, ia, (const T*)Bm, Cb,
                                                                                     (const T*)Rb, ib, scales, r_row0, (T*)out,
                                                                                     colstats_b, colstats_bucket);
        });
    } else {
        gmd_for_dtype(dtype, [&](auto tag) {
            using T = decltype(tag);
            concat_add_kernel<T><<<grid_for(rows * ((Ca + Cb) / cv)), kThreads, 0, s>>>((const T*)A, Ca, (const T*)Ra, ia, (const T*)Bm, Cb,
                                                                                       (const T*)Rb, ib, scales, r_row0, (T*)out, rows);
        });
    }
    GMD_CHECK_LAUNCH("gmd_concat_channels_add");
    return GMD_OK;
}

int gmd_silu(void* X, int dtype, int64_t n, gmd_stream_t stream) {
    GMD_REQUIRE(n >= 0, "gmd_silu: negative n");
    if (n == 0) return GMD_OK;
    GMD_REQUIRE(X && gmd_aligned16(X), "gmd_silu: null or unaligned pointer");
    GMD_REQUIRE(gmd_known_dtype(dtype), "gmd_silu: bad dtype %d", dtype);
    const int cv = gmd_is_half(dtype) ? 8 : 4;
    GMD_REQUIRE(n % cv == 0, "gmd_silu: n must be a multiple of %d", cv);
    gmd_for_dtype(dtype, [&](auto tag) {
        using T = decltype(tag);
        silu_kernel<T><<<grid_for(n / cv), kThreads, 0, (hipStream_t)stream>>>((T*)X, n / cv);
    });
    GMD_CHECK_LAUNCH("gmd_silu");
    return GMD_OK;
}

}  // extern "C"

GMD_WG_TRACE_SETTER(controlnet)
