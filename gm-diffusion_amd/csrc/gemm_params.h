// Parameter block of the dense-contraction kernels and the layout of a caller's workspace: plain C++ (no HIP), shared by the kernel
// translation units (gemm.hip, gemm_split.hip, through gemm_shared.h) and the host-only launch planner (gemm_plan.cpp).
#pragma once
#include <stdint.h>

namespace gmd {

constexpr int BK = 64;   // 16-bit elements per K step = 128 bytes = 8 chunks of 16 bytes
constexpr int BKS = 32;  // float32 elements per K step (gemm_split.hip) = 128 bytes

struct GemmParams {
    const void* A;
    const void* W;
    void* C;
    int M, N, K;
    int64_t lda, ldw, ldc, sA, sW, sC;
    const float* bias;
    const float* rowbias;
    int rows_per_group;
    int64_t ldrb;        // row stride of rowbias (>= N)
    const void* residual;
    int64_t ldr, sR;
    float alpha;
    int act;
    int out_f32;
    int c_split;       // float32 split path: store the output pre-split ([hi | lo] per 32 elements, GMD_F32SA as out_dtype; full-tile row epilogues)
    unsigned a_bytes, w_bytes;  // extents of the A / W operands (one batch slab) for the buffer descriptors
    int ksplit;          // > 1: grid z splits K; raw fp32 partial sums go to `ws` [ksplit][M][N], epilogue in splitk_reduce
    float* ws;
    // conv3x3 geometry (CONV instantiations only)
    int Hin, Win, Cin, Hout, Wout, stride, upsample, pad_lo;
    // conv3x3 K order of the ring kernel: channels are walked in blocks of `cblk` (a multiple of 64 dividing Cin), all nine
    // taps of a block before the next block.  cblk == Cin is the plain tap-major order.  A smaller block keeps the rows an
    // XCD re-reads for the next tap inside its 4 MiB L2 (see gmd_conv3x3).
    int cblk;
    // optional column statistics of the stored (rounded) output, for a following GroupNorm: {sum, sum of squares} over each
    // 64-row block and each bucket of `cs_bucket` adjacent columns -> colstats[M/64][N/cs_bucket][2] (ring kernel, row epilogue)
    float* colstats;
    int cs_bucket;
    // split-K only: leave the partial slabs in `ws` and do NOT launch the reduction (the consumer sums them:
    // gmd_conv3x3_groupnorm -> gn_slab_kernel of norm.hip)
    int defer_reduce;
    // tile order of the round-4 kernels inside an XCD's contiguous run of tiles: M-panels are walked in groups of `tile_group`
    // (m fastest inside a group, then the next N tile, then the next group); 1 = n fastest (the ring kernels' order).  Chosen on
    // the host so that what an XCD re-reads between reuses stays inside its 4 MiB L2 (gemm_plan.cpp: pick_tile_group).
    int tile_group;
    // fused Q|K|V projection (gmd_gemm_qkv_vt): column tiles from vt_col0 on are the V columns and leave TRANSPOSED, as the
    // attention kernels read them: vt_out[sample][column - vt_col0][token], row stride vt_ld, `vt_tokens` rows of C per sample
    void* vt_out;
    int vt_col0, vt_tokens;
    int64_t vt_ld;
    // in-kernel split-K reduction (round 5, splitk_fixup in gemm.hip): the K slices 0 .. ksplit-2 of a tile leave their accumulator
    // fragments in `ws` and count themselves in fix_cnt[tile]; the LAST slice (dispatched last) waits for them, adds them in slice
    // order and runs the fused epilogue -- no slab round trip, no reduction launch.  fix_bytes: extent of the fragment area.
    int fixup;
    unsigned fix_bytes;
    unsigned* fix_cnt;
    // conv3x3 K tail (gmd_conv3x3_tail; gemm_pp_kernel<CONV> only): behind the nine taps over Cin channels of A the K loop goes on over
    // K2 channels of a second operand A2, row-major [M, lda2] and read at the output pixel itself (a 1x1 tap): K = 9 Cin + K2, and W is
    // ONE matrix [N, 9 Cin + K2].  K2 == 0: no tail.  a2_bytes: extent of A2 for its buffer descriptor.
    const void* A2;
    int K2;
    int64_t lda2;
    unsigned a2_bytes;
    // nearest-2x upsampling conv3x3 as four 2x2 phase convolutions (gmd_conv3x3_up2; gemm_pp_kernel<CONV, TN, UP2> only).  Output
    // pixel (2i + py, 2j + px) reads the source pixels (i + a + py - 1, j + b + px - 1), a, b in {0, 1}, with the weights of the taps
    // that hit the same source pixel summed on the host: K = 4 Cin, W = [4][N][4 Cin], phase z = 2 py + px.  up2_rows = B Hin Win
    // GEMM rows per phase; M-panel mt of the launch is panel mt / 4 of phase mt % 4 (the phases of a panel are neighbours in the tile
    // order: they read the same source rows), M = 4 ceil(up2_rows / 256) 256 counts the panels' rows, the rows at or past up2_rows of a
    // phase's last panel are never loaded or stored.  Hout = 2 Hin, Wout = 2 Win.
    int up2;
    int up2_rows;
};

// The last GMD_WS_TAIL bytes of a caller's workspace hold the arrival counters of the in-kernel split-K reduction (one per tile):
// zero when the workspace is first handed to the library, left zero by every launch.  Slabs / fragments never reach into them.
constexpr int kFixupCounters = 16384;
constexpr int64_t kWsTail = (int64_t)kFixupCounters * 4;
static inline int64_t gmd_ws_usable_bytes(int64_t bytes) { return bytes > kWsTail ? bytes - kWsTail : 0; }

}  // namespace gmd
