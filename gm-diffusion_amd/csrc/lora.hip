// A LoRA adapter applied at run time: the rank update of one projection's output as ONE launch,
//   Y[m, n] <- round( float(Y[m, n]) + scales[index] * sum_j That[m, j] * Bw[n, j] ),   That[m, j] = round( sum_k X[m, k] * Aw[j, k] )
// Both sums in float32 on the matrix cores (16x16x32 MFMA), That rounded ONCE to the 16-bit type in between -- what a 16-bit PEFT model
// does between lora_A and lora_B -- the scale applied in float32 to the second accumulator, one rounding on the store.
//
// The launch moves M*K + 2*M*N elements for 2*M*Rp*(K + N) FLOP: it is bound by the read-modify-write of Y, so it is a streaming
// kernel (10 KB of LDS and 64 registers at rank <= 32, 35 KB and <= 144 at rank 128: several workgroups per CU), not a CU-owning one like gemm_pp_kernel.
//   * One workgroup = 4 waves = 64 rows.  Phase 1: wave w forms That for rows 16 w .. 16 w + 15 -- its X fragments come straight from
//     global memory (every X element is read by exactly one lane of the workgroup), the Aw tile [Rp][64] of each K step is shared
//     through LDS.  That goes to LDS as 16 bits (64 x Rp: at most 17 KB).
//   * Phase 2: the workgroup walks its range of N in tiles of 64 columns; the Bw tile [64][Rp] is staged through the LDS region the Aw
//     tiles used.  The A operand of an MFMA may take ANY row of the tile on a given lane, so a pair of MFMAs is fed rows
//     {8 q + i} and {8 q + 4 + i}: the lane then holds 8 CONSECUTIVE outputs of the contiguous dimension of Y and loads / stores Y
//     in whole 16-byte pieces.  Plain mode: the contiguous dimension is n (the Bw rows are the permuted operand); transposed mode
//     (Y [batch, N, ldy], the token contiguous): it is the token (the That rows are the permuted operand) and a workgroup's 64 rows
//     are 64 tokens of ONE batch entry.
//   * gridDim.y splits the N tiles when ceil(M / 64) workgroups cannot fill the chip; each workgroup then recomputes its That (Rp / N
//     of the work).  No atomics: every element of Y is written by exactly one lane, once.  Summation orders depend on k and j only,
//     never on the grid: a row's result is the same bits whatever else is in the launch.
// The scale is read from DEVICE memory (one wave-uniform load), so one captured graph serves every scale.
//
// The update of a feed-forward's first projection and its GEGLU as ONE launch (gmd_lora_geglu, MODE_GEGLU of the same kernel):
//   F[m, f] = round( v * gelu_erf(g) ),  v = float(Y[m, value(f)]) + s U[m, value(f)],  g = float(Y[m, gate(f)]) + s U[m, gate(f)]
// Y [M, N = 8C] is the pre-activation in the layout the interleaved ff1 weight produces: in a tile of 64 columns, columns 0-15 and
// 32-47 are the values of outputs 32 t .. 32 t + 31, columns 16-31 and 48-63 their gates; Bw's rows are in the same order.  Phase 1
// is the one above.  Phase 2 walks Y in those tiles; a tile takes four MFMA chains per wave (value / gate x two halves of its
// 32 outputs).  The A operand takes ANY row of the staged Bw tile on a given lane: chain (vg, q) is fed, on lane c, the Bw row of
// output f = 8 (c >> 2) + 4 q + (c & 3), so lane (c, g) holds value AND gate of the 8 CONSECUTIVE outputs 8 g .. 8 g + 7 of row
// 16 wid + c: two 16-byte loads of Y (whose 8 values and 8 gates are contiguous), one 16-byte store of F.  Y is read once and never
// written, every element of F is written once by one lane; v, g, the GELU and the product stay in float32.
//
// SEVERAL adapters on one projection as ONE launch (gmd_lora_update_stacked / gmd_lora_geglu_stacked, STACKED of the same kernel):
// Aw [Rp, K] and Bw [N, Rp] hold the adapters' factors side by side along the rank, the SUM of the ranks zero-padded to a multiple of
// 32, Rp in {32, 64, ..., 256}; instead of scales[index] the kernel reads a float32 ROW of column scales, colscales + index * ldc,
// Rp values long:
//   That[m, j] = round16( colscale[j] * sum_k X[m, k] * Aw[j, k] )      float32 accumulate, the scale applied in float32, ONE rounding
//   Y[m, n]   <- round16( float(Y[m, n]) + sum_j That[m, j] * Bw[n, j] )   float32 accumulate, one rounding on the store
//   GEGLU:     v, g as above with  U = sum_j That * Bw  (no further scale)
// The scale sits in front of That's one rounding: phase 2 -- the GEGLU's four MFMA chains included -- is the one above with s = 1, and
// the cost is four multiplies per 16-wide rank block per lane.  The row of column scales is read from DEVICE memory once per workgroup
// (thread j loads column j in front of the K loop and parks it in LDS; the lanes read their four columns per rank block back behind
// the loop), so one captured graph serves every weight setting and no register is held across the loop.  A column whose sum is exactly
// 0 -- every zero-padded column -- contributes exactly 0 whatever its table entry holds.  The summation orders are those of the
// single-adapter launch: they depend on k and j only, never on the grid.  Rp = 160 .. 256 instantiates the same template wider
// (45 - 72 KB of LDS, 116 - 190 VGPRs + 40 - 64 AGPRs, 2 - 3 waves per SIMD, no scratch: profiles/lora_multi.txt has the compiler's
// resource report); the LDS row strides TROW = Rp / 2 + 4 dwords fall on the residues 20, 36, 52 and 4 (mod 64 banks), exactly those
// of the widths up to 128, so the 16-byte row reads stay as conflict-free as they are there.
#include "gmd_common.h"

namespace {

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;

struct LoraParams {
    const bf16_t* X;
    const bf16_t* Aw;
    const bf16_t* Bw;
    bf16_t* Y;           // MODE_GEGLU: read-only
    bf16_t* F;           // MODE_GEGLU only: the output [M, N / 2], row stride ldf
    const float* scale;  // the entry this launch reads (array base + index); STACKED: its row of Rp column scales
    int M, K, N;
    int tokens, tblocks;  // transposed mode: tokens per batch entry, 64-token blocks per batch entry
    int ldx, ldy, ldf;    // elements
    int64_t strideY;      // transposed mode: elements between batch entries of Y
    int tiles_per_y;      // N tiles of 64 columns one workgroup walks
    unsigned xbytes, ybytes, fbytes;
};

enum { MODE_PLAIN = 0, MODE_TRANS = 1, MODE_GEGLU = 2 };

constexpr int ROWS = 64;  // rows of X per workgroup
constexpr int NT = 64;    // columns of Y per tile
constexpr int KT = 64;    // K step
constexpr int AROW = KT * 2 + 16;  // bytes per LDS row of an Aw tile: 36 dwords, conflict-free 16-byte row reads

template <typename HT, int RP, int MODE, bool STACKED = false>
__global__ __launch_bounds__(256) void lora_update_kernel(const LoraParams p) {
    GMD_WG_TRACE_SCOPE(WGK_OTHER);
    static_assert(RP <= 128 || STACKED, "ranks above 128 are stacked launches");
    constexpr bool TRANS = MODE == MODE_TRANS;
    constexpr int NJ = RP / 16;        // 16-wide blocks of the rank
    constexpr int NK2 = RP / 32;       // k-steps of the second product; also 16-byte staging chunks per thread and tile
    constexpr int TROW = RP * 2 + 16;  // bytes per LDS row of That and of a Bw tile: 20 / 36 / 52 / 68 (stacked: ... / 132) dwords, conflict-free 16-byte row reads
    constexpr int kStage = (RP * AROW > NT * TROW) ? RP * AROW : NT * TROW;
    __shared__ __attribute__((aligned(16))) unsigned char smem[kStage + ROWS * TROW + (STACKED ? RP * 4 : 0)];
    unsigned char* stage = smem;
    unsigned char* Ts = smem + kStage;
    float* cs = reinterpret_cast<float*>(smem + kStage + ROWS * TROW);  // STACKED: the row of column scales

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int c = lane & 15, g = lane >> 4;
    auto as_u4 = [](auto v) { return __builtin_bit_cast(uint4, v); };

    // rows of this workgroup: plain mode rows [row0, row0 + 64) of X; transposed mode tokens [tok0, tok0 + 64) of batch entry bidx
    int bidx = 0, tok0 = 0, row0;
    if (TRANS) {
        bidx = blockIdx.x / p.tblocks;
        tok0 = (blockIdx.x - bidx * p.tblocks) * ROWS;
        row0 = bidx * p.tokens + tok0;
    } else {
        row0 = blockIdx.x * ROWS;
    }
    const int rows_valid = TRANS ? min(ROWS, p.tokens - tok0) : min(ROWS, p.M - row0);

    // ---- phase 1: That = round(X Aw^T) for the 64 rows ----
    const __amdgpu_buffer_rsrc_t rsX = __builtin_amdgcn_make_buffer_rsrc((void*)p.X, 0, (int)p.xbytes, 0x00020000);
    const int xr = 16 * wid + c;  // this lane's row of the workgroup (B operand column)
    // a row beyond the valid ones falls outside the descriptor's range and reads as zeros
    const unsigned xoff = xr < rows_valid ? (unsigned)(((row0 + xr) * p.ldx + 8 * g) * 2) : 0x7fffffffu;
    // Two register sets of (Aw tile chunks, X fragments), loaded TWO K steps ahead of their use: at the low-resolution levels
    // (M = 512: one workgroup per CU) nothing else hides the latency of a load, and a K loop of 20 steps that waits for each step's
    // load in turn is most of the launch.  (ext-vector values, not the uint4 struct: a struct copy between address spaces would keep
    // an array in scratch)
    u32x4 ar0[NK2], ar1[NK2];
    uint4 x0[2], x1[2];
    // Aw [RP][K]: every chunk exists (the host pads the rank with zero rows); thread chunk u = row (tid + 256 u) >> 3, 16-byte slot & 7
    const bf16_t* a_src = p.Aw + (int64_t)(tid >> 3) * p.K + 8 * (tid & 7);
    unsigned char* a_dst = stage + (tid >> 3) * AROW + (tid & 7) * 16;
    auto load_set = [&](int k0, u32x4 (&ar)[NK2], uint4 (&xs)[2]) {
#pragma unroll
        for (int u = 0; u < NK2; ++u) ar[u] = *reinterpret_cast<const u32x4*>(a_src + (int64_t)(32 * u) * p.K + k0);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
            xs[kk] = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rsX, (int)(xoff < 0x7fffffffu ? xoff + (unsigned)((k0 + 32 * kk) * 2) : xoff), 0, 0));
    };
    f32x4 tacc[NJ];
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb) tacc[jb] = f32x4{0.f, 0.f, 0.f, 0.f};
    auto k_step = [&](int k0, u32x4 (&ar)[NK2], uint4 (&xs)[2]) {
#pragma unroll
        for (int u = 0; u < NK2; ++u) *reinterpret_cast<u32x4*>(a_dst + 32 * u * AROW) = ar[u];
        __syncthreads();
        const uint4 xf[2] = {xs[0], xs[1]};
        // this set's next use is two steps on (behind the last step it loads the last tile again: no branch around the loads, and
        // a set loaded that way is never used)
        load_set(min(k0 + 2 * KT, p.K - KT), ar, xs);
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int jb = 0; jb < NJ; ++jb) {
                // A: Aw[j = 16 jb + c][k0 + 32 kk + 8 g ..], B: X[row xr][the same k]: D row j = 16 jb + 4 g + i, column = row xr
                const uint4 af = *reinterpret_cast<const uint4*>(stage + (16 * jb + c) * AROW + (32 * kk + 8 * g) * 2);
                tacc[jb] = Half<HT>::mfma16(af, xf[kk], tacc[jb]);
            }
        __syncthreads();  // the tile is consumed: the next step may overwrite it
    };
    float csv = 0.f;  // STACKED: thread j brings column j's scale (RP <= 256 threads); visible behind the first K step's barrier
    if (STACKED && tid < RP) csv = p.scale[tid];
    load_set(0, ar0, x0);
    load_set(min(KT, p.K - KT), ar1, x1);
    if (STACKED && tid < RP) cs[tid] = csv;
    for (int k0 = 0; k0 < p.K; k0 += 2 * KT) {
        k_step(k0, ar0, x0);
        if (k0 + KT < p.K) k_step(k0 + KT, ar1, x1);
    }
    // the ONE rounding of That: row xr, columns 16 jb + 4 g + (0..3)
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb) {
        if constexpr (STACKED) {  // the column scale in float32 in front of the rounding; an exact 0 (a padded column) stays 0
            const float4 sc = *reinterpret_cast<const float4*>(cs + 16 * jb + 4 * g);
            const float scv[4] = {sc.x, sc.y, sc.z, sc.w};
#pragma unroll
            for (int i = 0; i < 4; ++i) tacc[jb][i] = tacc[jb][i] == 0.f ? 0.f : scv[i] * tacc[jb][i];
        }
        uint2 w;
        w.x = Half<HT>::pack2(tacc[jb][0], tacc[jb][1]);
        w.y = Half<HT>::pack2(tacc[jb][2], tacc[jb][3]);
        *reinterpret_cast<uint2*>(Ts + xr * TROW + (16 * jb + 4 * g) * 2) = w;
    }

    if constexpr (MODE == MODE_GEGLU) {
        // ---- phase 2 of the GEGLU launch: the walk over the 64-column tiles of Y (N % 64 == 0: every tile and every Bw row exists) ----
        const int t_begin = blockIdx.y * p.tiles_per_y, t_end = min(p.N / NT, t_begin + p.tiles_per_y);
        u32x4 breg[NK2];
        auto load_b = [&](int n0) {
#pragma unroll
            for (int u = 0; u < NK2; ++u) {
                const int id = tid + 256 * u, row = id / (RP / 8), ch = id - row * (RP / 8);
                breg[u] = *reinterpret_cast<const u32x4*>(p.Bw + (int64_t)(n0 + row) * RP + 8 * ch);
            }
        };
        auto store_b = [&]() {
#pragma unroll
            for (int u = 0; u < NK2; ++u) {
                const int id = tid + 256 * u, row = id / (RP / 8), ch = id - row * (RP / 8);
                *reinterpret_cast<u32x4*>(stage + row * TROW + ch * 16) = breg[u];
            }
        };
        if (t_begin < t_end) load_b(t_begin * NT);
        __syncthreads();  // That complete; the stage is free

        uint4 tf[NK2];  // That row xr, the B operand of every chain, held for the whole walk
#pragma unroll
        for (int ks = 0; ks < NK2; ++ks) tf[ks] = *reinterpret_cast<const uint4*>(Ts + xr * TROW + (32 * ks + 8 * g) * 2);
        const float s = STACKED ? 1.f : *p.scale;  // STACKED: the scales are in That already (1 * u folds to u)
        const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)p.Y, 0, (int)p.ybytes, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsF = __builtin_amdgcn_make_buffer_rsrc((void*)p.F, 0, (int)p.fbytes, 0x00020000);
        const bool valid = xr < rows_valid;
        // unsigned: the row may lie beyond M (unused then)
        const unsigned yrow = (unsigned)(row0 + xr) * (unsigned)p.ldy * 2u, frow = (unsigned)(row0 + xr) * (unsigned)p.ldf * 2u;

        for (int t = t_begin; t < t_end; ++t) {
            store_b();
            __syncthreads();
            load_b(min(t + 1, t_end - 1) * NT);  // the next tile into registers (the last tile loads its own again)
            // outputs 32 t + 8 g .. + 7: their values at tile columns 32 (g >> 1) + 8 (g & 1) .., their gates 16 columns on
            const unsigned yoff = yrow + (unsigned)(t * NT + 32 * (g >> 1) + 8 * (g & 1)) * 2u;
            uint4 yv = make_uint4(0, 0, 0, 0), yg = make_uint4(0, 0, 0, 0);
            if (valid) {
                yv = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rsY, (int)yoff, 0, 0));
                yg = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rsY, (int)(yoff + 32u), 0, 0));
            }
            f32x4 acc[2][2];  // [value / gate][q]: element i of chain q is output 8 g + 4 q + i
#pragma unroll
            for (int vg = 0; vg < 2; ++vg)
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    acc[vg][q] = f32x4{0.f, 0.f, 0.f, 0.f};
                    const int f = 8 * (c >> 2) + 4 * q + (c & 3);
                    const int brow = 32 * (f >> 4) + (f & 15) + 16 * vg;
#pragma unroll
                    for (int ks = 0; ks < NK2; ++ks) {
                        const uint4 bf = *reinterpret_cast<const uint4*>(stage + brow * TROW + (32 * ks + 8 * g) * 2);
                        acc[vg][q] = Half<HT>::mfma16(bf, tf[ks], acc[vg][q]);
                    }
                }
            if (valid) {
                const unsigned wv[4] = {yv.x, yv.y, yv.z, yv.w}, wg[4] = {yg.x, yg.y, yg.z, yg.w};
                unsigned o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float vlo, vhi, glo, ghi;
                    Half<HT>::unpack2(wv[e], vlo, vhi);
                    Half<HT>::unpack2(wg[e], glo, ghi);
                    const f32x4& av = acc[0][e >> 1];
                    const f32x4& ag = acc[1][e >> 1];
                    const int i = 2 * (e & 1);
                    o[e] = Half<HT>::pack2((vlo + s * av[i]) * gelu_erf(glo + s * ag[i]), (vhi + s * av[i + 1]) * gelu_erf(ghi + s * ag[i + 1]));
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, make_uint4(o[0], o[1], o[2], o[3])), rsF,
                                                       (int)(frow + (unsigned)(t * (NT / 2) + 8 * g) * 2u), 0, 0);
            }
            __syncthreads();  // the tile is consumed: the next store_b may overwrite it
        }
        return;
    }

    // ---- phase 2: the walk over N ----
    const int ntiles = (p.N + NT - 1) / NT;
    const int t_begin = blockIdx.y * p.tiles_per_y, t_end = min(ntiles, t_begin + p.tiles_per_y);
    u32x4 breg[NK2];
    auto load_b = [&](int n0) {  // Bw [N][RP]: rows at and beyond N are staged as zeros
#pragma unroll
        for (int u = 0; u < NK2; ++u) {
            const int id = tid + 256 * u, row = id / (RP / 8), ch = id - row * (RP / 8);
            u32x4 v = {0u, 0u, 0u, 0u};
            if (n0 + row < p.N) v = *reinterpret_cast<const u32x4*>(p.Bw + (int64_t)(n0 + row) * RP + 8 * ch);
            breg[u] = v;
        }
    };
    auto store_b = [&]() {
#pragma unroll
        for (int u = 0; u < NK2; ++u) {
            const int id = tid + 256 * u, row = id / (RP / 8), ch = id - row * (RP / 8);
            *reinterpret_cast<u32x4*>(stage + row * TROW + ch * 16) = breg[u];
        }
    };
    if (t_begin < t_end) load_b(t_begin * NT);
    __syncthreads();  // That complete (transposed mode reads other waves' rows); the stage is free

    // That fragments, held for the whole walk.  Plain: the B operand, row 16 wid + c.  Transposed: the A operand of MFMA h of the pair,
    // row (token) 32 (wid & 1) + 8 (c >> 2) + 4 h + (c & 3): lane (c, g) then holds tokens 32 (wid & 1) + 8 g + 4 h + i.
    constexpr int NTF = TRANS ? 2 : 1;
    uint4 tf[NTF][NK2];
#pragma unroll
    for (int h = 0; h < NTF; ++h) {
        const int trow = TRANS ? 32 * (wid & 1) + 8 * (c >> 2) + 4 * h + (c & 3) : xr;
#pragma unroll
        for (int ks = 0; ks < NK2; ++ks) tf[h][ks] = *reinterpret_cast<const uint4*>(Ts + trow * TROW + (32 * ks + 8 * g) * 2);
    }
    const float s = STACKED ? 1.f : *p.scale;  // STACKED: the scales are in That already (1 * u folds to u)
    const __amdgpu_buffer_rsrc_t rsY = __builtin_amdgcn_make_buffer_rsrc((void*)(TRANS ? p.Y + (int64_t)bidx * p.strideY : p.Y), 0, (int)p.ybytes, 0x00020000);

    for (int t = t_begin; t < t_end; ++t) {
        const int n0 = t * NT;
        store_b();
        __syncthreads();
        load_b(min(t + 1, t_end - 1) * NT);  // the next tile into registers (the last tile loads its own again)
        // the two 16-byte pieces of Y this lane owns in the tile
        unsigned yoff[2];
        int nvalid[2];  // elements of the piece that exist (8 = whole piece, <= 0 = none)
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (TRANS) {
                const int n = n0 + 32 * (wid >> 1) + 16 * q + c, tok = tok0 + 32 * (wid & 1) + 8 * g;
                nvalid[q] = n < p.N ? min(8, p.tokens - tok) : 0;
                yoff[q] = ((unsigned)n * (unsigned)p.ldy + (unsigned)tok) * 2u;  // unsigned: n may lie beyond N (piece unused then)
            } else {
                const int n = n0 + 32 * q + 8 * g;
                nvalid[q] = (xr < rows_valid && n < p.N) ? 8 : 0;  // N % 8 == 0: a piece exists whole or not at all
                yoff[q] = ((unsigned)(row0 + xr) * (unsigned)p.ldy + (unsigned)n) * 2u;  // unsigned: the row may lie beyond M (unused then)
            }
        }
        uint4 yv[2];
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            yv[q] = make_uint4(0, 0, 0, 0);
            if (nvalid[q] == 8) yv[q] = as_u4(__builtin_amdgcn_raw_buffer_load_b128(rsY, (int)yoff[q], 0, 0));
        }
        f32x4 acc[2][2];
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                acc[q][h] = f32x4{0.f, 0.f, 0.f, 0.f};
                // plain: A = Bw rows 32 q + 8 (c >> 2) + 4 h + (c & 3), B = That row xr -> D[n = 32 q + 8 g + 4 h + i][row xr]
                // transposed: A = That (permuted tokens, above), B = Bw row 32 (wid >> 1) + 16 q + c -> D[token 8 g + 4 h + i][that n]
                const int brow = TRANS ? 32 * (wid >> 1) + 16 * q + c : 32 * q + 8 * (c >> 2) + 4 * h + (c & 3);
#pragma unroll
                for (int ks = 0; ks < NK2; ++ks) {
                    const uint4 bf = *reinterpret_cast<const uint4*>(stage + brow * TROW + (32 * ks + 8 * g) * 2);
                    acc[q][h] = TRANS ? Half<HT>::mfma16(tf[h][ks], bf, acc[q][h]) : Half<HT>::mfma16(bf, tf[0][ks], acc[q][h]);
                }
            }
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            if (nvalid[q] == 8) {
                const unsigned w[4] = {yv[q].x, yv[q].y, yv[q].z, yv[q].w};
                unsigned o[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float lo, hi;
                    Half<HT>::unpack2(w[e], lo, hi);
                    const f32x4& a = acc[q][e >> 1];
                    o[e] = Half<HT>::pack2(lo + s * a[2 * (e & 1)], hi + s * a[2 * (e & 1) + 1]);
                }
                __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(u32x4, make_uint4(o[0], o[1], o[2], o[3])),
                                                       rsY, (int)yoff[q], 0, 0);
            } else if (TRANS && nvalid[q] > 0) {
                // the last piece of a token row that is no multiple of 8: element by element, the pad columns are not touched
                HT* yp = reinterpret_cast<HT*>(p.Y) + (int64_t)bidx * p.strideY + (yoff[q] >> 1);
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    if (e < nvalid[q]) Elem<HT>::st(yp + e, Elem<HT>::ld(yp + e) + s * acc[q][e >> 2][e & 3]);
            }
        }
        __syncthreads();  // the tile is consumed: the next store_b may overwrite it
    }
}

template <typename HT, int RP, bool STACKED>
void launch_lora(const LoraParams& p, int mode, dim3 grid, hipStream_t s) {
    if (mode == MODE_TRANS) lora_update_kernel<HT, RP, MODE_TRANS, STACKED><<<grid, 256, 0, s>>>(p);
    else if (mode == MODE_GEGLU) lora_update_kernel<HT, RP, MODE_GEGLU, STACKED><<<grid, 256, 0, s>>>(p);
    else lora_update_kernel<HT, RP, MODE_PLAIN, STACKED><<<grid, 256, 0, s>>>(p);
}

// the single-adapter launches: exactly the instantiations (and so the code objects) they have always been
template <typename HT>
void dispatch_lora(const LoraParams& p, int Rp, int mode, dim3 grid, hipStream_t s) {
    switch (Rp) {
        case 32: return launch_lora<HT, 32, false>(p, mode, grid, s);
        case 64: return launch_lora<HT, 64, false>(p, mode, grid, s);
        case 96: return launch_lora<HT, 96, false>(p, mode, grid, s);
        default: return launch_lora<HT, 128, false>(p, mode, grid, s);
    }
}

template <typename HT>
void dispatch_lora_stacked(const LoraParams& p, int Rp, int mode, dim3 grid, hipStream_t s) {
    switch (Rp) {
        case 32: return launch_lora<HT, 32, true>(p, mode, grid, s);
        case 64: return launch_lora<HT, 64, true>(p, mode, grid, s);
        case 96: return launch_lora<HT, 96, true>(p, mode, grid, s);
        case 128: return launch_lora<HT, 128, true>(p, mode, grid, s);
        case 160: return launch_lora<HT, 160, true>(p, mode, grid, s);
        case 192: return launch_lora<HT, 192, true>(p, mode, grid, s);
        case 224: return launch_lora<HT, 224, true>(p, mode, grid, s);
        default: return launch_lora<HT, 256, true>(p, mode, grid, s);
    }
}

// N tiles of 64 columns one workgroup walks: N is split over gridDim.y where the row blocks alone cannot fill the chip (256 CUs,
// several workgroups each); That is recomputed per split
int tiles_per_y(int64_t gx, int ntiles) {
    int nsplit = (int)((512 + gx - 1) / gx);
    if (nsplit > ntiles) nsplit = ntiles;
    if (nsplit < 1) nsplit = 1;
    return (ntiles + nsplit - 1) / nsplit;
}

// The table argument of both families: `table` + `index` is the one scale of a single-adapter launch; of a stacked launch
// (ldc >= 0) `table` + index * ldc is its row of Rp column scales.
struct ScaleArg {
    const float* table;
    int index;
    int64_t ldc;  // < 0: a single-adapter launch
    bool stacked() const { return ldc >= 0; }
    const float* entry() const { return stacked() ? table + (int64_t)index * ldc : table + index; }
};

int check_rank_and_table(const char* fn, int Rp, const ScaleArg& sa) {
    const int max_rp = sa.stacked() ? 256 : 128;
    GMD_REQUIRE(Rp > 0 && Rp % 32 == 0, "%s: padded rank Rp=%d must be a positive multiple of 32", fn, Rp);
    GMD_REQUIRE(Rp <= max_rp, "%s: padded rank Rp=%d above %d", fn, Rp, max_rp);
    if (sa.stacked()) {
        GMD_REQUIRE(sa.table != nullptr && sa.index >= 0, "%s: colscales must be a device array, the index non-negative", fn);
        GMD_REQUIRE(sa.ldc >= Rp, "%s: ldc=%lld smaller than Rp=%d", fn, (long long)sa.ldc, Rp);
    } else {
        GMD_REQUIRE(sa.table != nullptr && sa.index >= 0, "%s: scales must be a device array, the index non-negative", fn);
    }
    return GMD_OK;
}

int lora_geglu_impl(const char* fn, const void* X, const void* Aw, const void* Bw, const void* Y, void* F, int dtype, int M, int C, int Rp,
                    int64_t ldx, int64_t ldy, int64_t ldf, const ScaleArg& sa, gmd_stream_t stream) {
    if (dtype != GMD_BF16 && dtype != GMD_F16) {
        gmd_set_error("%s: GMD_BF16 / GMD_F16 are implemented (float32 composes gmd_gemm_nt twice, gmd_scaled_add and "
                      "gmd_geglu / gmd_geglu_interleaved)", fn);
        return GMD_ERR_UNSUPPORTED;
    }
    GMD_REQUIRE(M >= 0 && C > 0, "%s: bad shape M=%d C=%d", fn, M, C);
    GMD_REQUIRE(C % 64 == 0, "%s: C=%d must be a multiple of 64", fn, C);
    GMD_REQUIRE(C <= (1 << 24), "%s: C=%d too large", fn, C);
    if (int rc = check_rank_and_table(fn, Rp, sa)) return rc;
    const int N = 8 * C, NF = 4 * C;
    GMD_REQUIRE(ldx >= C && ldy >= N && ldf >= NF, "%s: ldx=%lld / ldy=%lld / ldf=%lld smaller than C=%d / 8C / 4C", fn, (long long)ldx,
                (long long)ldy, (long long)ldf, C);
    GMD_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0 && ldf % 8 == 0, "%s: leading dimensions must be multiples of 8", fn);
    if (M == 0) return GMD_OK;  // nothing to write
    GMD_REQUIRE(X && Aw && Bw && Y && F, "%s: null pointer", fn);
    GMD_REQUIRE(gmd_aligned16(X) && gmd_aligned16(Aw) && gmd_aligned16(Bw) && gmd_aligned16(Y) && gmd_aligned16(F),
                "%s: pointers must be 16-byte aligned", fn);
    const int64_t xbytes = (((int64_t)M - 1) * ldx + C) * 2, ybytes = (((int64_t)M - 1) * ldy + N) * 2, fbytes = (((int64_t)M - 1) * ldf + NF) * 2;
    GMD_REQUIRE(xbytes < (1ll << 31) && ybytes < (1ll << 31) && fbytes < (1ll << 31), "%s: X, Y or F exceeds 2 GiB (32-bit byte offsets)", fn);
    {
        const uintptr_t f0 = (uintptr_t)F, f1 = f0 + (uintptr_t)fbytes, x0 = (uintptr_t)X, x1 = x0 + (uintptr_t)xbytes, y0 = (uintptr_t)Y,
                        y1 = y0 + (uintptr_t)ybytes;
        GMD_REQUIRE(x1 <= f0 || f1 <= x0, "%s: F overlaps X", fn);
        GMD_REQUIRE(y1 <= f0 || f1 <= y0, "%s: F overlaps Y", fn);
    }
    LoraParams p;
    p.X = (const bf16_t*)X; p.Aw = (const bf16_t*)Aw; p.Bw = (const bf16_t*)Bw; p.Y = (bf16_t*)const_cast<void*>(Y);
    p.F = (bf16_t*)F; p.ldf = (int)ldf; p.fbytes = (unsigned)fbytes;
    p.scale = sa.entry();
    p.M = M; p.K = C; p.N = N;
    p.tokens = M; p.tblocks = 0;
    p.ldx = (int)ldx; p.ldy = (int)ldy;
    p.strideY = 0;
    p.xbytes = (unsigned)xbytes; p.ybytes = (unsigned)ybytes;
    const int64_t gx = ((int64_t)M + ROWS - 1) / ROWS;
    const int ntiles = N / NT;
    p.tiles_per_y = tiles_per_y(gx, ntiles);
    dim3 grid((unsigned)gx, (unsigned)((ntiles + p.tiles_per_y - 1) / p.tiles_per_y), 1);
    hipStream_t s = (hipStream_t)stream;
    if (sa.stacked()) dtype == GMD_F16 ? dispatch_lora_stacked<f16_t>(p, Rp, MODE_GEGLU, grid, s) : dispatch_lora_stacked<bf16_t>(p, Rp, MODE_GEGLU, grid, s);
    else dtype == GMD_F16 ? dispatch_lora<f16_t>(p, Rp, MODE_GEGLU, grid, s) : dispatch_lora<bf16_t>(p, Rp, MODE_GEGLU, grid, s);
    GMD_CHECK_LAUNCH(fn);
    return GMD_OK;
}

int lora_update_impl(const char* fn, const void* X, const void* Aw, const void* Bw, void* Y, int dtype, int M, int K, int Rp, int N, int64_t ldx,
                     int64_t ldy, int transposed, int batch, int tokens, int64_t strideY, const ScaleArg& sa, gmd_stream_t stream) {
    if (dtype != GMD_BF16 && dtype != GMD_F16) {
        gmd_set_error("%s: GMD_BF16 / GMD_F16 are implemented (float32 composes gmd_gemm_nt twice and gmd_scaled_add)", fn);
        return GMD_ERR_UNSUPPORTED;
    }
    GMD_REQUIRE(M >= 0 && K > 0 && N > 0, "%s: bad shape M=%d K=%d N=%d", fn, M, K, N);
    GMD_REQUIRE(K % 64 == 0, "%s: K=%d must be a multiple of 64", fn, K);
    if (int rc = check_rank_and_table(fn, Rp, sa)) return rc;
    if (transposed) {
        GMD_REQUIRE(batch > 0 && tokens > 0 && (int64_t)batch * tokens == M, "%s: transposed mode needs M=%d == batch=%d * tokens=%d", fn,
                    M, batch, tokens);
        GMD_REQUIRE(ldy >= ((int64_t)tokens + 7) / 8 * 8, "%s: ldy=%lld must cover tokens=%d rounded up to 8", fn, (long long)ldy, tokens);
        GMD_REQUIRE(strideY >= (int64_t)N * ldy && strideY % 8 == 0, "%s: strideY=%lld must cover N*ldy and be a multiple of 8", fn,
                    (long long)strideY);
    } else {
        GMD_REQUIRE(N % 8 == 0, "%s: N=%d must be a multiple of 8 (16-byte pieces of Y)", fn, N);
        GMD_REQUIRE(ldy >= N, "%s: ldy=%lld smaller than N=%d", fn, (long long)ldy, N);
    }
    if (M == 0) return GMD_OK;  // nothing to write
    GMD_REQUIRE(X && Aw && Bw && Y, "%s: null pointer", fn);
    GMD_REQUIRE(gmd_aligned16(X) && gmd_aligned16(Aw) && gmd_aligned16(Bw) && gmd_aligned16(Y), "%s: pointers must be 16-byte aligned", fn);
    GMD_REQUIRE(ldx % 8 == 0 && ldy % 8 == 0, "%s: leading dimensions must be multiples of 8", fn);
    GMD_REQUIRE(ldx >= K, "%s: ldx=%lld smaller than K=%d", fn, (long long)ldx, K);
    const int64_t xbytes = (((int64_t)M - 1) * ldx + K) * 2;
    const int64_t yslab = transposed ? (((int64_t)N - 1) * ldy + (tokens + 7) / 8 * 8) * 2 : (((int64_t)M - 1) * ldy + N) * 2;
    const int64_t ybytes = transposed ? ((int64_t)batch - 1) * strideY * 2 + yslab : yslab;
    GMD_REQUIRE(xbytes < (1ll << 31) && yslab < (1ll << 31), "%s: X or a batch entry of Y exceeds 2 GiB (32-bit byte offsets)", fn);
    {
        const uintptr_t x0 = (uintptr_t)X, x1 = x0 + (uintptr_t)xbytes, y0 = (uintptr_t)Y, y1 = y0 + (uintptr_t)ybytes;
        GMD_REQUIRE(x1 <= y0 || y1 <= x0, "%s: X overlaps Y", fn);
    }
    LoraParams p;
    p.X = (const bf16_t*)X; p.Aw = (const bf16_t*)Aw; p.Bw = (const bf16_t*)Bw; p.Y = (bf16_t*)Y;
    p.scale = sa.entry();
    p.M = M; p.K = K; p.N = N;
    p.tokens = transposed ? tokens : M;
    p.tblocks = (p.tokens + ROWS - 1) / ROWS;
    p.ldx = (int)ldx; p.ldy = (int)ldy;
    p.strideY = transposed ? strideY : 0;
    p.F = nullptr; p.ldf = 0; p.fbytes = 0;
    p.xbytes = (unsigned)xbytes; p.ybytes = (unsigned)yslab;
    const int64_t gx = transposed ? (int64_t)batch * p.tblocks : ((int64_t)M + ROWS - 1) / ROWS;
    GMD_REQUIRE(gx < (1ll << 31), "%s: grid too large", fn);
    const int ntiles = (N + NT - 1) / NT;
    p.tiles_per_y = tiles_per_y(gx, ntiles);
    dim3 grid((unsigned)gx, (unsigned)((ntiles + p.tiles_per_y - 1) / p.tiles_per_y), 1);
    hipStream_t s = (hipStream_t)stream;
    const int mode = transposed ? MODE_TRANS : MODE_PLAIN;
    if (sa.stacked()) dtype == GMD_F16 ? dispatch_lora_stacked<f16_t>(p, Rp, mode, grid, s) : dispatch_lora_stacked<bf16_t>(p, Rp, mode, grid, s);
    else dtype == GMD_F16 ? dispatch_lora<f16_t>(p, Rp, mode, grid, s) : dispatch_lora<bf16_t>(p, Rp, mode, grid, s);
    GMD_CHECK_LAUNCH(fn);
    return GMD_OK;
}

}  // namespace

extern "C" int gmd_lora_geglu(const void* X, const void* Aw, const void* Bw, const void* Y, void* F, int dtype, int M, int C, int Rp,
                              int64_t ldx, int64_t ldy, int64_t ldf, const float* scales, int index, gmd_stream_t stream) {
    return lora_geglu_impl("gmd_lora_geglu", X, Aw, Bw, Y, F, dtype, M, C, Rp, ldx, ldy, ldf, ScaleArg{scales, index, -1}, stream);
}

extern "C" int gmd_lora_geglu_stacked(const void* X, const void* Aw, const void* Bw, const void* Y, void* F, int dtype, int M, int C, int Rp,
                                      int64_t ldx, int64_t ldy, int64_t ldf, const float* colscales, int index, int64_t ldc,
                                      gmd_stream_t stream) {
    GMD_REQUIRE(ldc >= 0, "gmd_lora_geglu_stacked: ldc=%lld smaller than Rp=%d", (long long)ldc, Rp);
    return lora_geglu_impl("gmd_lora_geglu_stacked", X, Aw, Bw, Y, F, dtype, M, C, Rp, ldx, ldy, ldf, ScaleArg{colscales, index, ldc}, stream);
}

extern "C" int gmd_lora_update(const void* X, const void* Aw, const void* Bw, void* Y, int dtype, int M, int K, int Rp, int N, int64_t ldx,
                               int64_t ldy, int transposed, int batch, int tokens, int64_t strideY, const float* scales, int index,
                               gmd_stream_t stream) {
    return lora_update_impl("gmd_lora_update", X, Aw, Bw, Y, dtype, M, K, Rp, N, ldx, ldy, transposed, batch, tokens, strideY,
                            ScaleArg{scales, index, -1}, stream);
}

extern "C" int gmd_lora_update_stacked(const void* X, const void* Aw, const void* Bw, void* Y, int dtype, int M, int K, int Rp, int N,
                                       int64_t ldx, int64_t ldy, int transposed, int batch, int tokens, int64_t strideY,
                                       const float* colscales, int index, int64_t ldc, gmd_stream_t stream) {
    GMD_REQUIRE(ldc >= 0, "gmd_lora_update_stacked: ldc=%lld smaller than Rp=%d", (long long)ldc, Rp);
    return lora_update_impl("gmd_lora_update_stacked", X, Aw, Bw, Y, dtype, M, K, Rp, N, ldx, ldy, transposed, batch, tokens, strideY,
                            ScaleArg{colscales, index, ldc}, stream);
}

GMD_WG_TRACE_SETTER(lora)
