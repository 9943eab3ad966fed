// Launch planning of the dense contractions and the plan queries of the C ABI (gemm_plan.h).  Plain C++: no HIP, no GPU.
#include "gemm_plan.h"
#include <stdio.h>
#include <stdlib.h>

namespace gmd {

namespace {

inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }  // (64-bit: M + bm - 1 overflows an int from M = 2^31 - bm on)
inline int64_t tile_count(const Plan& pl, int M, int N) { return cdiv(M, pl.bm) * cdiv(N, pl.bn); }

// Kernel-tuning override (debug only: tools/, never the product path).  It takes effect only in a process that has
// GMD_TUNING=1 in its environment -- both the GMD_GEMM_FORCE seed read when the library is loaded and the in-process
// gmd_gemm_plan_override() -- and every forced plan still passes plan_unsupported() below, the ONE place that refuses a
// kernel lacking the epilogue a launch asks for (round 2: five memory-access faults of tools/bench_graph_ops.py under forced
// odd-TN ring tiles, whose plain epilogue stored [M, N] into the [M, N/2] output of the fused-GEGLU projection).
bool tuning_enabled() {
    const char* t = getenv("GMD_TUNING");
    return t && t[0] == '1';
}

PlanConfig g_cfg = load_plan_config();  // read once when the library is loaded
thread_local int t_plan_family = 0;

}  // namespace

PlanConfig load_plan_config() {
    PlanConfig c{};
    const bool tuning = tuning_enabled();
    const char* e;
    if (tuning && (e = getenv("GMD_GEMM_FORCE"))) sscanf(e, "%d,%d,%d,%d", &c.force.bm, &c.force.bn, &c.force.pf, &c.force.ks);
    // GMD_PP=0 keeps the round-3 plans (A/B measurements of whole runs)
    e = getenv("GMD_PP");
    c.pp_enabled = !(e && e[0] == '0');
    // Plan family (round 5, see make_plan): 0 = the plan that is fastest launch by launch when the launch has the chip to itself (direct
    // calls, single-stream pipelines, the VAE); 1 = the co-running family -- 256-row tiles everywhere, filled up with K slices -- for
    // launches that share the chip with a second stream's kernels (the dual-UNet pipeline's two forwards).  The calling thread selects
    // it with gmd_gemm_plan_family(); GMD_PP=b / GMD_PP=1 pin family 1 / 0 for the whole process (A/B runs).
    c.family_pin = (e && e[0] == 'b') ? 1 : ((e && e[0] == '1') ? 0 : -1);
    // K slices of the co-running family: until about f1_target workgroups, at least f1_min_steps K steps each (GMD_F1_TARGET /
    // GMD_F1_MIN_STEPS: whole-run A/B only).  The target was 256 -- one workgroup per CU -- until the end of round 5; HALF the chip is
    // better: 256 -> 128: 761.5 -> 744.5 ms per batch (-2.2 %, 3 of 3 interleaved rounds), 1320.4 -> 1307.3 at batch 8 (-1.0 %); 160 / 144:
    // 747.7 / 746.3; 112: 766.8 (the 80-tile projections lose their second slice); 96 / 64 / 32: 768.9 / 780.3 / 813.8; 320: +4.4 %
    // (profiles/r05_ab_f1_slice_target.txt).  Fewer slices = fewer prologues, fragment round trips and finisher waits per product: CU-time,
    // which is what two forwards sharing the chip pay for; the other stream fills the CUs a launch leaves free.
    e = getenv("GMD_F1_TARGET");
    c.f1_target = e ? atoi(e) : 128;
    e = getenv("GMD_F1_MIN_STEPS");
    c.f1_min_steps = e ? atoi(e) : 8;
    e = getenv("GMD_F1_BN128");  // GMD_F1_BN128=0: A/B
    c.f1_bn128 = !(e && e[0] == '0');
    // In-kernel split-K reduction up to this many K slices (0 = off: slabs + reduction launch everywhere)
    e = getenv("GMD_SPLITK_FIXUP");
    c.fixup_max = e ? atoi(e) : 4;
    // How stride-1 convolutions on 256-row ping-pong tiles fetch their activations: 0 (default since the end of round 5) = per-tap implicit
    // GEMM (gemm_pp_kernel<CONV>); 2 = input patch resident in LDS, continuous consumers (conv_patch_cont_kernel); 1 = patch resident,
    // ping-pong consumers (conv_patch_kernel).  GMD_CONV_PATCH seeds it when the library is loaded; gmd_conv_patch_override() changes it
    // in-process for A/B runs and tests (GMD_TUNING=1 only).  Whole-run A/Bs: round 4 (launch-by-launch plans) 838.7 / 840.6 / 837.5 ms for
    // 0 / 1 / 2 -- level, and the patch forms pull half the bytes from L2 (25.6 instead of 52 KB per K step), so 2 became the default; at
    // the end of round 5 (co-running plan family, in-kernel reduction, the shorter epilogue) the per-tap kernel is 1.0 % FASTER on the wall
    // of the two-stream pipeline (764.1 -> 756.4 ms, 4 of 4 interleaved rounds; 765.1 -> 756.8, 2 of 2), level with the streams serialised
    // (922.1 / 921.0) and at batch 8 (1266.6 / 1265.2), and level or ahead launch by launch (8x64x64 320->320 61.0 -> 58.4 us, 640->320
    // 113.7 -> 111.4): profiles/r05_ab_conv_patch_mode.txt.  The patch kernels stay in the library (tests, A/B).
    e = getenv("GMD_CONV_PATCH");
    c.conv_patch_mode = (e && e[0] >= '0' && e[0] <= '2') ? e[0] - '0' : 0;
    // The float32 loader / converter kernel (gemm_split_lc_kernel).  0 (default): never; -1: where it fits (GMD_SPLIT_LC=1); 1: wherever
    // it is instantiated (gmd_gemm_plan_override(.., pf = 244, ..); pf = 9: never).  NOT the default: alone on the chip it wins 3-9 % on
    // one-round launches, but in the two-stream float32 pipeline the whole run is 2.3 % SLOWER with it (bench.py tolerance_path 1894 ->
    // 1937 ms per batch): like the 16-bit loader-wave kernels it owns its CU (144 KB of LDS), and a workgroup of the other stream on the
    // same CU was already hiding what the loader waves hide.  Kept for single-stream users and as the measured
    // answer to "take the operand split out of the float32 main loop".
    e = getenv("GMD_SPLIT_LC");
    c.split_lc_mode = (e && e[0] == '1') ? -1 : 0;
    // experiments only (GMD_TUNING=1): GMD_CONV_CBLK=<multiple of 64 dividing Cin>
    e = tuning ? getenv("GMD_CONV_CBLK") : nullptr;
    c.conv_cblk = e ? atoi(e) : 0;
    return c;
}

PlanConfig plan_config() {
    PlanConfig c = g_cfg;
    c.family = c.family_pin >= 0 ? c.family_pin : t_plan_family;
    return c;
}

// The round-3 heuristic, shared by the 16-bit path (make_plan: with the override and the GEGLU pairing flag) and float32 on the matrix
// cores (f32_plan: neither; its K steps are 32 deep, but it slices like the 16-bit launch of the same shape).
// Tile / split-K selection.  All SD-1.5 channel widths (320, 640, 1280, 2560, 5120, 10240) are multiples of
// 160, the VAE widths (128, 256, 512) of 128.  Launches that would leave most of the 256 CUs idle and have a
// deep K (the 8x8 / 16x16 UNet levels: K up to 23040) are split along K.
Plan base_plan(int M, int N, int K, int batch, int64_t ws_bytes, bool pair_tiles, const Force& force) {
    Plan pl{64, 64, kRing, 1};  // kRing = LDS-DMA pipeline (fastest measured); 1/2 = register-staged fallbacks
    if (M >= 96 && N >= 96) {
        pl.bm = 128;
        pl.bn = (N % 160 == 0 && !pair_tiles) ? 160 : 128;  // GEGLU needs an even number of 16-column tiles per wave
    }
    // GMD_GEMM_FORCE="bm,bn,pf,ksplit" (0 = keep heuristic): tuning experiments only (tools/bench_gemm.py).  Parsed ONCE per process
    // -- the launch path itself never touches the environment; gmd_gemm_plan_override() changes it in-process for A/B runs.
    const int fbm = force.bm, fbn = force.bn, fpf = force.pf, fks = force.ks;
    if (fbm && fbn) { pl.bm = fbm; pl.bn = fbn; }
    if (fpf) pl.pf = fpf == kForceRing ? kRing : fpf;
    const int64_t tiles = tile_count(pl, M, N) * batch;
    const int nk = K / BK;
    if (batch == 1 && tiles < 160 && nk >= 24 && !pair_tiles) {  // K >= 1536: the slab reduction (a second launch) must pay for itself
        // whole waves of blocks: 512 (two per CU) when the tile grid is at least a quarter of the chip, else 256 (the
        // fp32 slab traffic of more slices costs more than the second resident block buys) -- measured, tools/bench_gemm.py
        int ks = (int)(((tiles >= 64 ? 512 : 256) + tiles / 2) / tiles);
        if (ks > nk / 8) ks = nk / 8;  // at least 8 K steps (512 channels) per slice
        if (ks > 16) ks = 16;
        if (ks > 1 && (int64_t)ks * M * N * (int64_t)sizeof(float) <= ws_bytes) pl.ksplit = ks;
    }
    // one workgroup per CU (224..256 large tiles) leaves every SIMD with a single wave; with a very deep K (>= 10240: the
    // 32x32 up-block convolutions over concatenated inputs) two slices -- two workgroups per CU -- pay for the slab reduction
    // (tools/bench_graph_ops.py: 1280->640 149.9 -> 137.0 us, 1920->640 208.6 -> 181.1 us; 640->640, K = 5760, loses)
    if (batch == 1 && pl.bm == 128 && tiles >= 224 && tiles <= 256 && nk >= 160 && !pair_tiles &&
        2 * (int64_t)M * N * (int64_t)sizeof(float) <= ws_bytes)
        pl.ksplit = 2;
    // batched, operand-swapped projections (V^T[b] = W_v x_b^T: M = channels <= 640, N = tokens): 128-row tiles leave a
    // ragged third row block at M = 320 and lose to 64x64 tiles even at M = 640 (tools/bench_vt.py: 27.9 -> 18.4 us, 17.2 -> 15.7 us)
    if (pl.ksplit == 1 && batch > 1 && M <= 640 && pl.bm == 128 && !pair_tiles && !(fbm && fbn)) {
        pl.bm = 64;
        pl.bn = 64;
    }
    if (pl.ksplit == 1 && tiles < 256 && pl.bm == 128 && !(fbm && fbn)) {  // cannot fill the chip: 4-5x more, smaller tiles
        pl.bm = 64;
        pl.bn = 64;
    }
    if (fks) pl.ksplit = ((int64_t)fks * M * N * (int64_t)sizeof(float) <= ws_bytes && batch == 1) ? fks : 1;
    return pl;
}

Plan make_plan(const PlanConfig& cfg, int M, int N, int K, int batch, int64_t ws_bytes, bool pair_tiles, bool want_cs) {
    Plan pl = base_plan(M, N, K, batch, ws_bytes, pair_tiles, cfg.force);
    const int nk = K / BK;
    // Round-4 kernels: one workgroup per CU with dedicated LDS-DMA loader waves (gemm_pp_kernel, kPingPong: 256-row tiles;
    // gemm_lc_kernel, kLoaderConsumer: 128- / 64-row tiles for launches with about one tile per CU).
    //
    // DEFAULT POLICY -- the plan that is fastest launch by launch (tools/sweep_pp.py --round3, device time inside a HIP graph: -11 % /
    // -15 % summed over the UNet's linear + convolution launches at batch 8 / 4 against the round-3 plans; every row of the vendor-
    // library yardstick, tools/vs_library_gemm.py):
    //   * ping-pong kernel where there are >= 256 tiles of 256 x 160 (every level-0 linear / convolution at batch 8), or of 256 x 128
    //     where N is not a multiple of 160 (VAE decoder); the GEGLU projection (value | gate pairs) from K = 1280 up, or K = 640 with
    //     at least 8192 rows;
    //   * loader / consumer kernel where 128- or 64-row tiles give 200...256 workgroups (with K slices where K is deep): conv 32x32
    //     640->640 at batch 8 72.8 -> 55.5 us, 64x64 320->320 at batch 4 41.3 -> 33.0 us, linear M=2048 N=1280 K=5120 49.4 -> 36.8 us.
    //     More than 256 such tiles would run in two rounds of one workgroup per CU, fewer than ~200 leave CUs idle: both keep the
    //     plans above.
    // CO-RUNNING FAMILY (gmd_gemm_plan_family(1); what the dual-UNet pipeline selects for its two overlapped forwards) -- the largest
    // tile, filled up with K slices: slower launch by launch, faster on the wall of the two-stream pipeline in every interleaved
    // whole-run A/B (profiles/r05_ab_plan_default.txt, five rounds on one box: 867.7 -> 849.0 ms per batch at batch 4 (-2.2 %, 5 of 5),
    // 1454.3 -> 1436.9 at batch 8 (-1.2 %, 3 of 3); round 4, three boxes: -0.4 ... -1.3 %).  With two streams in flight a second
    // workgroup is always there to hide a kernel's own latencies, so L2 -> LDS bytes per product -- (1/BM + 1/BN) x 2 B: 0.020 for a
    // 256 x 160 tile, 0.028 for 128 x 160, 0.044 for 64 x 160 -- weigh more than the launch's time alone on the chip.  With the
    // streams serialised the same family LOSES 8.6 % (1018.3 -> 1106.3 ms), so it is never the choice of a launch that runs alone:
    // family 0 stays the default of the C ABI.  GMD_PP=0: the round-3 plans.
    const Force& f = cfg.force;
    if (cfg.pp_enabled && batch == 1 && !(f.bm && f.bn) && !f.pf && !f.ks && M >= 64) {
        const int64_t mt256 = cdiv(M, 256);
        const int bn = N % 160 == 0 ? 160 : (N % 128 == 0 ? 128 : 0);
        if (cfg.family == 1) {
            if (pair_tiles) {
                if (M >= 256 && N % 128 == 0) pl = Plan{256, 128, kPingPong, 1};  // GEGLU pairs value / gate tiles: no K slices
            } else if (bn && M >= 256) {
                auto slices = [&](int bnc) {
                    const int64_t t = mt256 * (N / bnc);
                    int ks = t >= cfg.f1_target ? 1 : (int)((cfg.f1_target + t / 2) / t);
                    if (ks > 8) ks = 8;
                    while (ks > 1 && (nk / ks < cfg.f1_min_steps || (int64_t)ks * M * N * (int64_t)sizeof(float) > ws_bytes)) --ks;
                    return ks;
                };
                int bnc = bn;
                // 128-column tiles where they still fit ONE round of workgroups: their row segments are whole 128-byte lines (a
                // 160-column tile shares every third line of a row with its neighbour) and there are a quarter more of them
                // (not for a launch that is to emit GroupNorm statistics: their 10-channel buckets need 80-column wave tiles)
                if (cfg.f1_bn128 && !want_cs && bn == 160 && N % 128 == 0 && mt256 * (N / 128) * slices(128) <= 256) bnc = 128;
                pl = Plan{256, bnc, kPingPong, slices(bnc)};
            }
        } else if (pair_tiles) {
            if (M >= 256 && N % 128 == 0 && ((nk >= 20 && M >= 512) || (nk >= 10 && M >= 8192))) pl = Plan{256, 128, kPingPong, 1};
        } else if (bn && M >= 256 && mt256 * (N / bn) >= 256) {
            pl = Plan{256, bn, kPingPong, 1};
        } else if (bn) {
            bool found = false;
            for (int bm = 128; bm >= 64 && !found; bm >>= 1) {  // unsplit first: the larger tile wins when both fill the chip
                const int64_t t = cdiv(M, bm) * (N / bn);
                if (t >= 200 && t <= 256) { pl = Plan{bm, bn, kLoaderConsumer, 1}; found = true; }
            }
            // 64-row tiles pull 28 KB per K step through the CU for half the products of a 128-row tile (36 KB): with a deep K two
            // slices of 128-row tiles beat them (tools/sweep_lc.py, conv 16x16 1280->1280 at batch 8: 78.2 -> 66.9 us, 2560->1280:
            // 155 -> 121 us; at K = 5760 the slab reduction costs more than it buys: 39.4 vs 42.1 us)
            if (found && pl.bm == 64 && nk >= 144 && 2 * (int64_t)M * N * (int64_t)sizeof(float) <= ws_bytes) {
                const int64_t t = cdiv(M, 128) * (N / bn) * 2;
                if (t >= 200 && t <= 256) pl = Plan{128, bn, kLoaderConsumer, 2};
            }
            for (int bm = 128; bm >= 64 && !found; bm >>= 1) {  // K slices: at least 20 K steps (K = 1280) each
                const int64_t t = cdiv(M, bm) * (N / bn);
                for (int ks = 2; ks <= 8 && !found; ++ks)
                    if (t * ks >= 200 && t * ks <= 256 && nk / ks >= 20 && (int64_t)ks * M * N * (int64_t)sizeof(float) <= ws_bytes) {
                        pl = Plan{bm, bn, kLoaderConsumer, ks};
                        found = true;
                    }
            }
            // still nothing (the GM UNet's 16x16 projections at batch 4, M = 1024 N = K = 1280: 128 tiles of 64 x 160, K too short to
            // slice): 64 x 128 loader / consumer tiles, a quarter more workgroups than 64 x 160 (tools/dbg/sweep_rows.py: 13.7 us on the
            // legacy 64 x 64 kernel -> 11.3 us; the vendor library 11.5)
            if (!found && !want_cs && N % 128 == 0 && nk >= 8) {  // (validated for K >= 512 only)
                const int64_t t = cdiv(M, 64) * (N / 128);
                if (t >= 144 && t <= 256) pl = Plan{64, 128, kLoaderConsumer, 1};
            }
        }
    }
    return pl;
}

// float32 on the matrix cores: the round-3 heuristic without override; 128 x 160 / 128 x 128 tiles (two workgroups per CU) and 64 x 64
// for launches that cannot put 256 large tiles on the chip.  GEGLU pairs value / gate tiles inside a wave: even TN (128 x 128 or
// 64 x 64 tiles), unsplit K.
Plan f32_plan(int M, int N, int K, int batch, int64_t ws_bytes, bool geglu) {
    Plan pl = base_plan(M, N, K, batch, ws_bytes, false, Force{});
    if (geglu) {
        if (pl.bn == 160) pl.bn = 128;
        pl.ksplit = 1;
    }
    return pl;
}

// One 16-bit element type (bf16_t or f16_t): plan, kernel choice, split-K reduction.  float16 instantiates the kernels the
// heuristic actually picks; the register-staged and deeper-ring tuning variants exist for bfloat16 only (plan overrides).
// Column statistics (GemmParams::colstats) come out of the row epilogue of the default ring kernels only: every tile must be a
// full tile of a single, unsplit launch whose waves own 64 rows x (BN/2) columns, a whole number of buckets.
// A split-K launch reduces inside the kernel (splitk_fixup) when this holds; `ws_bytes` = usable workspace bytes.  The one predicate
// of the launch itself (launch_half) and of the plan queries that depend on it (column statistics).
// In-kernel split-K reduction (splitk_fixup) instead of slabs + splitk_reduce_kernel: the round-4 kernels (one workgroup per CU,
// wave tiles in registers), up to cfg.fixup_max slices (the finisher reads the other slices' fragments one after the other), the
// consumer of the slabs not being a fused GroupNorm (defer_reduce).  Bit-identical to the slab path (same order of additions).
int64_t fixup_bytes(const Plan& pl, int M, int N) { return (int64_t)(pl.ksplit - 1) * tile_count(pl, M, N) * pl.bm * pl.bn * 4; }
bool fixup_plan_ok(const PlanConfig& cfg, const Plan& pl, int M, int N, int64_t ws_bytes, bool defer_reduce) {
    if (pl.ksplit <= 1 || pl.ksplit > cfg.fixup_max || defer_reduce || ws_bytes <= 0 || !has_fixup(pl.pf)) return false;
    const int64_t frag_bytes = fixup_bytes(pl, M, N);
    return tile_count(pl, M, N) <= kFixupCounters && frag_bytes <= ws_bytes && frag_bytes < 0xFFFF0000LL;
}

// (split launches: the finisher of the in-kernel reduction runs the row epilogue of an unsplit launch, statistics included)
bool colstats_plan_ok(const PlanConfig& cfg, const Plan& pl, int M, int N, int batch, int bucket, int64_t ws_bytes) {
    return wave_owns_64_rows(pl) && (pl.bn == 160 || pl.bn == 128) && (pl.ksplit == 1 || fixup_plan_ok(cfg, pl, M, N, ws_bytes, false)) &&
           batch == 1 && bucket > 0 && M % pl.bm == 0 && N % pl.bn == 0 && (pl.bn / 2) % bucket == 0;
}

// The one place that refuses a plan (heuristic or forced) whose kernel lacks an epilogue the launch asks for; nullptr = fine.
//   * GEGLU pairs value / gate tiles of 16 columns inside a wave: only kernels with an EVEN number of column tiles per wave
//     implement it (128x128 and 64x64 register / DMA kernels, ring tiles with TN = 2 or 4) and never with split-K -- any
//     other kernel's plain epilogue would store [M, N] into the [M, N/2] output;
//   * column statistics come out of the full-tile row epilogue of the two default 128-row ring kernels only.
const char* plan_unsupported(const PlanConfig& cfg, const Plan& pl, const GemmParams& p, int batch, int64_t ws_bytes) {
    if (p.act == GMD_ACT_GEGLU) {
        if (!even_tn(pl) || pl.ksplit > 1 || p.out_f32 || (pl.pf == kLoaderConsumer && pl.bm != 128)) return "has no GEGLU epilogue";
    }
    if (p.colstats) {
        const bool rows_ok = !p.out_f32 && p.act != GMD_ACT_GEGLU && (p.ldc & 7) == 0 && (p.residual == nullptr || (p.ldr & 7) == 0) &&
                             (p.rowbias == nullptr || ((p.ldrb & 3) == 0 && (reinterpret_cast<uintptr_t>(p.rowbias) & 15) == 0));
        if (!rows_ok || p.defer_reduce || !colstats_plan_ok(cfg, pl, p.M, p.N, batch, p.cs_bucket, ws_bytes))
            return "cannot emit column statistics (they need the full-tile row epilogue of an unsplit 128-row ring launch: ask "
                   "gmd_gemm_colstats_plan first)";
    }
    return nullptr;
}

// Tile order of the ping-pong / loader-consumer kernels (GemmParams::tile_group).  Workgroups with equal id % 8 share an XCD and get
// a contiguous run of tiles; with n fastest an XCD walks whole M-panels, so between two uses of a weight tile lie all the others:
//   * weights larger than the activations (N > M: the GEGLU projections of the 16x16 / 8x8 levels, W up to 26 MB): m fastest --
//     each weight tile then goes to ONE XCD instead of all eight (rocprofv3 FETCH_SIZE, M=2048 N=10240 K=1280: 226 MB = 7.2x the
//     algorithmic reads with n fastest);
//   * activations larger, but the weights do not fit an XCD's 4 MiB L2 beside them (M=8192 N=5120 K=640: W = 6.5 MB, 231 MB fetched
//     = 13.6x): the XCD's M-panels are walked together, one N tile at a time, so every weight tile is fetched once per XCD.
// Everything else keeps n fastest.
int pick_tile_group(const Plan& pl, int M, int N, int K) {
    if (!is_loader_wave(pl.pf)) return 1;
    const int tiles_m = (int)cdiv(M, pl.bm);
    const int64_t w_bytes = (int64_t)N * K * 2;
    int g;
    if (N > M) g = tiles_m;
    else if (w_bytes <= (3ll << 20)) return 1;
    else g = (tiles_m + 7) / 8;  // the XCD's share of M-panels
    // Round 5: at most FOUR M-panels per group.  An XCD walks its run of tiles one W panel at a time over the group's A panels: the
    // A panels must survive in its 4 MiB L2 beside the W panels in flight and the output lines passing through, the W panels are
    // streamed once.  rocprofv3 FETCH_SIZE against the group (profiles/r05_pmc_tile_group.txt, MB read, algorithmic in brackets):
    // M=4096 N=5120 K=640 [11.8]: 16 (the N > M rule) 126, 8: 50, 4: 37.5, 2: 59;  M=2048 N=10240 K=1280 [31.5]: 8 (N > M) 145, 4: 110,
    // 2: 130;  M=8192 N=5120 K=640 [17]: 4 (the share rule) 66, 8: 84, 2: 121;  M=1024 N=10240 K=1280: 4 = all its panels, 63.
    if (g > 4) g = 4;
    return g < 1 ? 1 : g;
}

// fused Q|K|V projection with transposed V tiles (GemmParams::vt_out, epilogue_cols_vt): every tile full and through the row epilogue,
// the V columns starting on a tile boundary, wave tiles (64 or 32 rows) inside one sample
bool qkv_vt_plan_ok(const Plan& pl, int M, int N, int batch, int vt_col0, int vt_tokens) {
    return batch == 1 && pl.ksplit == 1 && M % pl.bm == 0 && N % pl.bn == 0 && vt_col0 > 0 && vt_col0 < N && vt_col0 % pl.bn == 0 &&
           vt_tokens > 0 && vt_tokens % 64 == 0 && M % vt_tokens == 0;
}

// ---- float32 on the matrix cores ----
// What the float32 row epilogues need: an unsplit launch of full 128-row tiles.  Column statistics, pre-split output and transposed V
// tiles all come out of them only.
bool f32_full_rows(const Plan& pl, int M, int N, int batch) {
    return pl.bm == 128 && pl.ksplit == 1 && batch == 1 && M % 128 == 0 && N % pl.bn == 0;
}

// producer column statistics (GemmParams::colstats): the waves own 64 rows x (BN/2) columns -- a whole number of buckets: the float32
// twin of colstats_plan_ok
bool f32_colstats_ok(int M, int N, int K, int batch, int64_t ws_bytes, int bucket) {
    if (M <= 0 || N <= 0 || K <= 0 || K % BKS || batch != 1 || bucket <= 0) return false;
    const Plan pl = f32_plan(M, N, K, batch, ws_bytes, false);
    return f32_full_rows(pl, M, N, batch) && (pl.bn / 2) % bucket == 0;
}

// the launch can store its result pre-split (GemmParams::c_split): the row epilogues write whole 4-element pieces of 32-element
// chunks (wave tiles start at multiples of 16 columns; GEGLU: of 8 output columns -- 64 / 80 wide)
bool f32_out_ok(int M, int N, int K, bool geglu, int64_t ws_bytes) {
    if (M <= 0 || N <= 0 || K <= 0 || K % BKS) return false;
    return f32_full_rows(f32_plan(M, N, K, 1, ws_bytes, geglu), M, N, 1);
}

// fused Q|K|V projection with transposed V tiles on the float32 matrix-core path (GemmParams::vt_out)
bool f32_qkv_vt_ok(int M, int N, int K, int vt_col0, int vt_tokens, int64_t ws_bytes) {
    if (M <= 0 || N <= 0 || K <= 0 || K % BKS || vt_col0 <= 0 || vt_col0 >= N || vt_tokens <= 0 || vt_tokens % 64 || M % vt_tokens) return false;
    const Plan pl = f32_plan(M, N, K, 1, ws_bytes, false);
    return f32_full_rows(pl, M, N, 1) && vt_col0 % pl.bn == 0;
}

// gmd_gemm_qkv_vt_ok / gmd_gemm_qkv_vt: either path (ws_bytes: the USABLE bytes, i.e. without the counter tail)
bool qkv_vt_ok(const PlanConfig& cfg, int dtype, int M, int N, int K, int vt_col0, int vt_tokens, int64_t ws_bytes) {
    if (dtype == GMD_F32SW || dtype == GMD_F32SA) return f32_qkv_vt_ok(M, N, K, vt_col0, vt_tokens, ws_bytes);
    if (!is_half(dtype) || M <= 0 || N <= 0 || K <= 0 || K % BK) return false;
    return qkv_vt_plan_ok(make_plan(cfg, M, N, K, 1, ws_bytes, false), M, N, 1, vt_col0, vt_tokens);
}

// the loader / converter kernel runs ONE workgroup per CU: taken when the launch's 128-row tiles come in (nearly) whole rounds of 256
bool split_lc_fits(const PlanConfig& cfg, const Plan& pl, int M, int N, int K, int batch) {
    if (cfg.split_lc_mode == 0 || batch != 1 || pl.bm != 128 || K / BKS < 4) return false;
    if (cfg.split_lc_mode == 1) return true;
    // measured (tools/ab_split_lc.py, bit-identical results): +3...+9 % where the launch is ONE round of workgroups (conv 8x32x32
    // 640->640 208 -> 196 us, 4x64x64 320->320 110 -> 102 us, linear M=8192 N=640 K=2560 101 -> 95 us); launches of several rounds lose
    // 10-28 % to two co-resident workgroups of the ring kernel, which overlap one tile's epilogue with the next one's prologue
    const int64_t tiles = cdiv(M, 128) * cdiv(N, pl.bn) * (pl.ksplit > 1 ? pl.ksplit : 1);
    return tiles >= 200 && tiles <= 256;
}

// ---- conv3x3 ----
// Channel block of the ring kernel's conv3x3 K order.  The tiles resident on one XCD (64 = 32 CUs x 2 workgroups, a
// contiguous run of the n-fastest tile order) read the same input rows once per filter tap; walking ALL channels of a tap
// before the next tap makes the re-read distance rows x Cin x 2 bytes, which for Cin >= 640 at 64x64 (5.2 MB) no longer
// fits the XCD's 4 MiB L2 (rocprofv3 FETCH_SIZE: 9.1x the algorithmic reads on 8x64x64 640->320,
// profiles/r01_pmc_conv_attention_current.txt).  Blocks of `cblk` channels bring the distance back under 3 MB
// (rocprofv3 after: 1.97x, 125.5 -> 118.8 us; profiles/r02_pmc_conv_gemm_traffic.txt).  Shapes whose rows already fit keep
// the tap-major order (cblk == Cin): at 2.6 MB (32x32, Cin 1280) the blocked order measured slower, not faster.
// `elem_bytes` / `step`: 2 / 64 for the 16-bit kernels, 4 / 32 for float32 on the matrix cores (one K step of channels).
int conv_channel_block(int B, int Hin, int Win, int Cin, int Cout, int elem_bytes, int step) {
    const int64_t rows_total = (int64_t)B * Hin * Win;
    const int tiles_n = (Cout + 159) / 160;
    const int64_t rows_resident = (int64_t)(64 / tiles_n > 0 ? 64 / tiles_n : 1) * 128;  // input rows under one XCD's resident tiles
    const int64_t rows = rows_total / 8 < rows_resident ? (rows_total + 7) / 8 : rows_resident;
    const int64_t budget = 3ll << 20;
    if (rows * Cin * elem_bytes <= budget) return Cin;
    int best = step;
    for (int d = step; d < Cin; d += step)
        if (Cin % d == 0 && rows * d * elem_bytes <= budget) best = d;
    return best;
}
int conv_channel_block(const PlanConfig& cfg, int B, int Hin, int Win, int Cin, int Cout, int dtype) {
    if (dtype == GMD_F32) return Cin;  // the exact kernel walks tap-major
    if (is_split(dtype)) return conv_channel_block(B, Hin, Win, Cin, Cout, 4, BKS);
    if (cfg.conv_cblk >= BK && cfg.conv_cblk % BK == 0 && Cin % cfg.conv_cblk == 0) return cfg.conv_cblk;
    return conv_channel_block(B, Hin, Win, Cin, Cout, 2, BK);
}

// conv_patch_kernel: stride-1 / pad-1 convolutions whose 256-pixel tiles are whole image rows (or whole images) -- every UNet level
bool conv_patch_ok(const GemmParams& p) {
    const int H = p.Hin, W = p.Win, HW = H * W;
    if (p.stride != 1 || p.upsample || p.pad_lo != 1 || p.Hout != H || p.Wout != W) return false;
    if (W < 8 || W > 64 || (W & (W - 1)) || p.Cin % BK || p.M % HW) return false;
    if (HW >= 256 ? (HW % 256 != 0) : (256 % HW != 0)) return false;
    const int R = HW >= 256 ? 256 / W : H, nimg = 256 / (R * W);
    return nimg * (R + 2) * (W + 2) <= 400;
}
// ping-pong structure with the input patch resident in LDS (conv_patch_kernel): same tiles, same epilogues, same plan code
bool use_conv_patch(const PlanConfig& cfg, const Plan& pl, const GemmParams& p) {
    return pl.pf == kPingPong && cfg.conv_patch_mode != 0 && conv_patch_ok(p) && (int64_t)pl.ksplit <= p.Cin / BK;
}

// `upsample`: 0, 1 (nearest 2x) or GMD_UPSAMPLE_TO(Hout, Wout) (nearest to a given size; include/gmd_hip.h).  False (message left
// for the caller's error) when the requested size is not one a stride-2 level can have come from: Hout in {2 Hin - 1, 2 Hin}.  For
// those two torch's nearest map with size= is dst >> 1, as for 2x: only the bound of the virtual image moves (the kernels test
// uy >= Hout), and Hout <= 2 Hin keeps uy >> 1 inside the source.  `upsample` leaves as 0 / 1.
bool conv_out_shape(int Hin, int Win, int stride, int& upsample, int pad_mode, int& Hout, int& Wout, int& pad_lo) {
    if (upsample == 1) { Hout = 2 * Hin; Wout = 2 * Win; pad_lo = 1; }
    else if (upsample) {
        Hout = upsample >> 16; Wout = upsample & 0xFFFF; pad_lo = 1;
        if (upsample < 0 || !(Hout == 2 * (int64_t)Hin - 1 || Hout == 2 * (int64_t)Hin) || !(Wout == 2 * (int64_t)Win - 1 || Wout == 2 * (int64_t)Win)) {
            gmd_set_error("gmd_conv3x3: upsample to %dx%d from %dx%d: each output side must be 2*in - 1 or 2*in", Hout, Wout, Hin, Win);
            return false;
        }
        upsample = 1;
    }
    else if (pad_mode == 1) { Hout = (Hin + 1 - 3) / 2 + 1; Wout = (Win + 1 - 3) / 2 + 1; pad_lo = 0; }
    else { Hout = (Hin + 2 - 3) / stride + 1; Wout = (Win + 2 - 3) / stride + 1; pad_lo = 1; }
    return true;
}

// split-K factor the conv launch will use (1 = unsplit); the same planners the launch itself calls
int conv_plan_ksplit(const PlanConfig& cfg, int dtype, int64_t M, int Cin, int Cout, int64_t ws_bytes) {
    if (is_split(dtype)) return f32_plan((int)M, Cout, 9 * Cin, 1, ws_bytes, false).ksplit;
    if (is_half(dtype)) return make_plan(cfg, (int)M, Cout, 9 * Cin, 1, ws_bytes, false).ksplit;
    return 1;
}

// Nearest-2x upsampling conv3x3 as four 2x2 phase convolutions: see gemm_plan.h.  make_plan is asked as for any GEMM of these
// dimensions (no plan of an existing launch changes); a split the in-kernel reduction cannot take (more slices than fixup_max, no
// workspace) is cut down, since the phase epilogue has no slab form.
bool up2_plan(const PlanConfig& cfg, int dtype, int B, int Hin, int Win, int Cin, int Cout, int bucket, int64_t ws_bytes, Plan& pl, int& M) {
    if (!is_half(dtype) || B <= 0 || Hin <= 0 || Win <= 0 || Cin <= 0 || Cout <= 0 || Cin % BK || bucket < 0) return false;
    const int64_t rows = (int64_t)B * Hin * Win, mv = 4 * cdiv(rows, 256) * 256;
    // 32-bit row indices and buffer offsets: output rows, the input and the four weight slabs
    if (mv >= (1LL << 31) || rows * Cin * 2 >= 0xFFFF0000LL || 16LL * Cout * Cin * 2 >= 0xFFFF0000LL) return false;
    M = (int)mv;
    pl = make_plan(cfg, M, Cout, 4 * Cin, 1, ws_bytes, false, bucket > 0);
    if (!(pl.pf == kPingPong && pl.bm == 256 && (pl.bn == 160 || pl.bn == 128)) || Cout % pl.bn) return false;
    if (pl.ksplit > 1 && !fixup_plan_ok(cfg, pl, M, Cout, ws_bytes, false)) {
        pl.ksplit = cfg.fixup_max >= 2 && pl.ksplit > cfg.fixup_max ? cfg.fixup_max : 1;
        if (pl.ksplit > 1 && !fixup_plan_ok(cfg, pl, M, Cout, ws_bytes, false)) pl.ksplit = 1;
    }
    // statistics: 64-row wave tiles inside one sample, whole buckets per wave tile (80 or 64 columns)
    if (bucket > 0 && (((int64_t)Hin * Win) % 64 || (pl.bn / 2) % bucket)) return false;
    return true;
}

}  // namespace gmd

// ---- the planner's part of the C ABI: overrides and plan queries ----
using namespace gmd;

namespace {
const char kTuningOnly[] = "%s: kernel-tuning overrides are a debug facility; set GMD_TUNING=1 in the environment to use them";
}

extern "C" {

int gmd_gemm_plan_override(int bm, int bn, int pf, int ksplit) {
    if (!(bm >= 0 && bn >= 0 && pf >= 0 && ksplit >= 0)) {
        gmd_set_error("gmd_gemm_plan_override: negative value");
        return GMD_ERR_INVALID;
    }
    if (!tuning_enabled() && (bm | bn | pf | ksplit) != 0) {
        gmd_set_error(kTuningOnly, "gmd_gemm_plan_override");
        return GMD_ERR_UNSUPPORTED;
    }
    g_cfg.force = Force{bm, bn, pf, ksplit};
    // the float32 matrix-core path takes the kernel family only of an override: kLoaderConsumer = its loader / converter kernel
    // wherever instantiated, anything else = its default (the in-register split)
    g_cfg.split_lc_mode = pf == kLoaderConsumer ? 1 : 0;
    return GMD_OK;
}

int gmd_gemm_plan_family(int family) {
    const int prev = t_plan_family;
    if (family == 0 || family == 1) t_plan_family = family;  // anything else: query only
    return prev;
}

int gmd_splitk_fixup_max(int max_slices) {
    const int prev = g_cfg.fixup_max;
    if (max_slices >= 0) g_cfg.fixup_max = max_slices > 16 ? 16 : max_slices;
    return prev;
}

int gmd_conv_patch_override(int mode) {
    if (!(mode >= 0 && mode <= 2)) {
        gmd_set_error("gmd_conv_patch_override: mode 0, 1 or 2");
        return GMD_ERR_INVALID;
    }
    if (!tuning_enabled()) {
        gmd_set_error(kTuningOnly, "gmd_conv_patch_override");
        return GMD_ERR_UNSUPPORTED;
    }
    g_cfg.conv_patch_mode = mode;
    return GMD_OK;
}

// (every query: the tail of the workspace holds the split-K arrival counters)
int gmd_gemm_colstats_plan(int dtype, int M, int N, int K, int batch, int64_t workspace_bytes, int bucket) {
    const int64_t ws = gmd_ws_usable_bytes(workspace_bytes);
    if (is_split(dtype)) return f32_colstats_ok(M, N, K, batch, ws, bucket);  // round 4
    if (!is_half(dtype) || M <= 0 || N <= 0 || K <= 0 || K % BK != 0) return 0;
    const PlanConfig cfg = plan_config();
    return colstats_plan_ok(cfg, make_plan(cfg, M, N, K, batch, ws, false, true), M, N, batch, bucket, ws) ? 1 : 0;
}

int gmd_gemm_plan_info(int dtype, int M, int N, int K, int batch, int64_t workspace_bytes, int geglu, int* out4) {
    if (!(is_half(dtype) && M > 0 && N > 0 && K > 0 && K % BK == 0 && batch > 0 && out4)) {
        gmd_set_error("gmd_gemm_plan_info: 16-bit launches only");
        return GMD_ERR_INVALID;
    }
    const Plan pl = make_plan(plan_config(), M, N, K, batch, gmd_ws_usable_bytes(workspace_bytes), geglu != 0);
    out4[0] = pl.bm; out4[1] = pl.bn; out4[2] = pl.pf; out4[3] = pl.ksplit;
    return GMD_OK;
}

// 1 when gmd_conv3x3_up2 of these dimensions launches (out4, when given: tile rows, tile columns, kernel code, K slices)
int gmd_conv3x3_up2_plan(int dtype, int B, int Hin, int Win, int Cin, int Cout, int colstats_bucket, int64_t workspace_bytes, int* out4) {
    Plan pl{};
    int M = 0;
    if (!up2_plan(plan_config(), dtype, B, Hin, Win, Cin, Cout, colstats_bucket, gmd_ws_usable_bytes(workspace_bytes), pl, M)) return 0;
    if (out4) { out4[0] = pl.bm; out4[1] = pl.bn; out4[2] = pl.pf; out4[3] = pl.ksplit; }
    return 1;
}

// K slices of a float32 matrix-core (GMD_F32S / GMD_F32SW / GMD_F32SA) gmd_gemm_nt launch: slabs + splitk_reduce_f32_kernel when > 1
int gmd_split_plan_ksplit(int M, int N, int K, int64_t workspace_bytes) {
    if (M <= 0 || N <= 0 || K <= 0 || K % BKS) return 0;
    return f32_plan(M, N, K, 1, gmd_ws_usable_bytes(workspace_bytes), false).ksplit;
}

// Which kernel a float32 matrix-core launch takes: the planner calls of launch_split_any (gemm_split.hip), in its order.  A batched
// launch gets no workspace (gmd_gemm_nt hands none over), so it never slices K.
int gmd_split_plan_info(int dtype, int M, int N, int K, int batch, int64_t workspace_bytes, int geglu, int* out4) {
    if (!(is_split(dtype) && M > 0 && N > 0 && K > 0 && K % BKS == 0 && batch > 0 && out4)) {
        gmd_set_error("gmd_split_plan_info: float32 matrix-core launches only (GMD_F32S / GMD_F32SW / GMD_F32SA, K a multiple of %d)", BKS);
        return GMD_ERR_INVALID;
    }
    const Plan pl = f32_plan(M, N, K, batch, batch == 1 ? gmd_ws_usable_bytes(workspace_bytes) : 0, geglu != 0);
    const bool lc = dtype == GMD_F32SW && split_lc_fits(plan_config(), pl, M, N, K, batch);  // pre-split weights, plain activations
    out4[0] = pl.bm; out4[1] = pl.bn; out4[2] = lc ? kLoaderConsumer : kRing; out4[3] = pl.ksplit;
    return GMD_OK;
}

// 1 when a float32-split gmd_gemm_nt launch of these dimensions can take out_dtype = GMD_F32SA (store its result pre-split)
int gmd_gemm_out_split_ok(int M, int N, int K, int geglu, int64_t workspace_bytes) {
    return f32_out_ok(M, N, K, geglu != 0, gmd_ws_usable_bytes(workspace_bytes));
}

int gmd_gemm_qkv_vt_ok(int dtype, int M, int N, int K, int vt_col0, int vt_tokens, int64_t workspace_bytes) {
    return qkv_vt_ok(plan_config(), dtype, M, N, K, vt_col0, vt_tokens, gmd_ws_usable_bytes(workspace_bytes));
}

}  // extern "C"
