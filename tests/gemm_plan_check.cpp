// Stand-alone check of the planner decisions the C ABI does not expose (csrc/gemm_plan.cpp): tile order, conv channel block, in-kernel
// reduction, patch geometry, the float32 loader / converter kernel.  tests/test_gemm_plan_cpu.py compiles it together with
// gemm_plan.cpp and gmd_error.cpp under -fsanitize=address,undefined and runs it: any failed check or sanitizer report fails the test.
#include <stdio.h>
#include <initializer_list>
#include "../gm-diffusion_amd/csrc/gemm_plan.h"

using namespace gmd;

static int failures = 0;
#define CHECK(cond)                                                   \
    do {                                                              \
        if (!(cond)) {                                                \
            printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++failures;                                               \
        }                                                             \
    } while (0)

static GemmParams conv_params(int B, int H, int W, int Cin, int Cout) {
    GemmParams p{};
    p.M = B * H * W; p.N = Cout; p.K = 9 * Cin;
    p.Hin = p.Hout = H; p.Win = p.Wout = W; p.Cin = Cin; p.stride = 1; p.pad_lo = 1;
    return p;
}

// every plan the sweep sees: slabs inside the workspace, fragments inside the 32-bit extent of their buffer descriptor
static void check_plan(const PlanConfig& cfg, const Plan& pl, int M, int N, int K, int batch, int64_t ws) {
    CHECK(pl.ksplit >= 1 && pl.bm > 0 && pl.bn > 0);
    if (pl.ksplit > 1) CHECK((int64_t)pl.ksplit * M * N * 4 <= ws && batch == 1);
    for (bool defer : {false, true})
        if (fixup_plan_ok(cfg, pl, M, N, ws, defer)) CHECK(!defer && has_fixup(pl.pf) && fixup_bytes(pl, M, N) < 0xFFFF0000LL && fixup_bytes(pl, M, N) <= ws);
    const int g = pick_tile_group(pl, M, N, K);
    CHECK(g >= 1 && g <= 4);
    if (!is_loader_wave(pl.pf)) CHECK(g == 1);
    colstats_plan_ok(cfg, pl, M, N, batch, 10, ws);
    qkv_vt_plan_ok(pl, M, N, batch, N / 3 * 2, 64);
}

int main() {
    PlanConfig cfg = load_plan_config();
    const Plan pp160{256, 160, kPingPong, 1}, pp128{256, 128, kPingPong, 1};

    // tile order: the groups of profiles/r05_pmc_tile_group.txt, and n fastest where the weights fit beside the activations
    CHECK(pick_tile_group(pp128, 4096, 5120, 640) == 4);
    CHECK(pick_tile_group(pp128, 2048, 10240, 1280) == 4);
    CHECK(pick_tile_group(pp128, 8192, 5120, 640) == 4);
    CHECK(pick_tile_group(pp160, 8192, 320, 320) == 1 && pick_tile_group(pp160, 32768, 1280, 1152) == 1);  // 0.2 / 2.8 MiB of weights
    CHECK(pick_tile_group(pp160, 8192, 1280, 1228) == 1 && pick_tile_group(pp160, 8192, 1280, 1229) == 4);  // 3 MiB = N x 1228.8 x 2 B
    CHECK(pick_tile_group(Plan{128, 160, kRing, 1}, 2048, 10240, 1280) == 1);                              // ring kernels: always n fastest

    // conv channel block: blocked where an XCD's rows no longer fit its L2, tap-major where they do; exact float32 walks tap-major
    CHECK(conv_channel_block(cfg, 8, 64, 64, 640, 320, GMD_BF16) < 640);
    CHECK(640 % conv_channel_block(cfg, 8, 64, 64, 640, 320, GMD_BF16) == 0 && conv_channel_block(cfg, 8, 64, 64, 640, 320, GMD_BF16) % 64 == 0);
    CHECK(conv_channel_block(cfg, 8, 32, 32, 1280, 1280, GMD_BF16) == 1280);
    CHECK(conv_channel_block(cfg, 8, 64, 64, 640, 320, GMD_F32) == 640);
    CHECK(conv_channel_block(cfg, 8, 64, 64, 640, 320, GMD_F32SW) == conv_channel_block(8, 64, 64, 640, 320, 4, 32));
    CHECK(conv_channel_block(8, 64, 64, 640, 320, 4, 32) < conv_channel_block(8, 64, 64, 640, 320, 2, 64));  // 4-byte rows: half the channels
    {
        PlanConfig forced = cfg;  // GMD_CONV_CBLK applies to the 16-bit path only, and only where it divides Cin in whole K steps
        forced.conv_cblk = 128;
        CHECK(conv_channel_block(forced, 8, 32, 32, 1280, 1280, GMD_F16) == 128);
        CHECK(conv_channel_block(forced, 8, 32, 32, 1280, 1280, GMD_F32S) == conv_channel_block(cfg, 8, 32, 32, 1280, 1280, GMD_F32S));
        forced.conv_cblk = 96;
        CHECK(conv_channel_block(forced, 8, 32, 32, 1280, 1280, GMD_F16) == 1280);
    }

    // patch geometry: power-of-two widths 8..64 whose 256-pixel tiles are whole rows / images
    for (int W : {8, 16, 32, 64}) CHECK(conv_patch_ok(conv_params(8, W, W, 320, 320)));
    CHECK(!conv_patch_ok(conv_params(8, 30, 30, 320, 320)));
    CHECK(!conv_patch_ok(conv_params(8, 128, 128, 320, 320)));
    {
        PlanConfig patch = cfg;
        const GemmParams p = conv_params(8, 64, 64, 320, 320);
        CHECK(!use_conv_patch(cfg, pp160, p));  // mode 0 is the default
        patch.conv_patch_mode = 2;
        CHECK(use_conv_patch(patch, pp160, p) && !use_conv_patch(patch, Plan{128, 160, kLoaderConsumer, 1}, p));
        CHECK(!use_conv_patch(patch, Plan{256, 160, kPingPong, 8}, p));  // more K slices than channel blocks (320 / 64)
    }

    // float32 loader / converter kernel: off by default; where it fits = one round of 128-row tiles; forced = wherever instantiated
    {
        const Plan pl{128, 160, kRing, 1};
        PlanConfig lc = cfg;
        CHECK(!split_lc_fits(cfg, pl, 8192, 640, 2560, 1));
        lc.split_lc_mode = -1;
        CHECK(split_lc_fits(lc, pl, 8192, 640, 2560, 1));       // 64 x 4 = 256 tiles
        CHECK(!split_lc_fits(lc, pl, 32768, 640, 2560, 1));     // several rounds
        CHECK(!split_lc_fits(lc, pl, 8192, 640, 2560, 2) && !split_lc_fits(lc, Plan{64, 64, kRing, 1}, 8192, 640, 2560, 1));
        CHECK(!split_lc_fits(lc, pl, 8192, 640, 96, 1));        // fewer than 4 K steps
        lc.split_lc_mode = 1;
        CHECK(split_lc_fits(lc, pl, 32768, 640, 2560, 1));
    }

    // gmd_split_plan_info: the plan query of the float32 matrix-core launches answers what f32_plan + split_lc_fits answer
    {
        const int64_t whole = (96ll << 20) + kWsTail;
        int o[4] = {-1, -1, -1, -1};
        auto is = [&](int bm, int bn, int code, int ks) { return o[0] == bm && o[1] == bn && o[2] == code && o[3] == ks; };
        for (int dtype : {GMD_F32S, GMD_F32SW, GMD_F32SA}) {
            CHECK(gmd_split_plan_info(dtype, 4096, 1280, 64, 1, whole, 0, o) == GMD_OK && is(128, 160, 0, 1));     // 256 tiles
            CHECK(gmd_split_plan_info(dtype, 4096, 1024, 64, 1, whole, 0, o) == GMD_OK && is(128, 128, 0, 1));
            CHECK(gmd_split_plan_info(dtype, 300, 200, 320, 1, whole, 0, o) == GMD_OK && is(64, 64, 0, 1));
            CHECK(gmd_split_plan_info(dtype, 256, 320, 2560, 1, whole, 0, o) == GMD_OK && is(128, 160, 0, 5));
            CHECK(gmd_split_plan_info(dtype, 64, 320, 2048, 1, whole, 0, o) == GMD_OK && is(64, 64, 0, 4));
            CHECK(gmd_split_plan_info(dtype, 4096, 1280, 10240, 1, whole, 0, o) == GMD_OK && is(128, 160, 0, 2));  // the reducer's second lap
            CHECK(gmd_split_plan_info(dtype, 256, 320, 2560, 1, kWsTail, 0, o) == GMD_OK && is(64, 64, 0, 1));     // no usable workspace
            CHECK(gmd_split_plan_info(dtype, 256, 320, 2560, 8, whole, 0, o) == GMD_OK && is(64, 64, 0, 1));       // batched: never sliced
            CHECK(gmd_split_plan_info(dtype, 4096, 2560, 320, 1, whole, 1, o) == GMD_OK && is(128, 128, 0, 1));    // GEGLU: even TN
            CHECK(gmd_split_plan_info(dtype, 4096, 1280, 48, 1, whole, 0, o) == GMD_ERR_INVALID);                  // K % 32
            CHECK(gmd_split_plan_info(dtype, 4096, 1280, 64, 1, whole, 0, nullptr) == GMD_ERR_INVALID);
        }
        for (int dtype : {GMD_F32, GMD_BF16, GMD_F16, 6, -1}) CHECK(gmd_split_plan_info(dtype, 4096, 1280, 64, 1, whole, 0, o) == GMD_ERR_INVALID);
        CHECK(gmd_split_plan_ksplit(256, 320, 2560, whole) == 5 && gmd_split_plan_ksplit(4096, 1280, 10240, whole) == 2);
    }

    // in-kernel reduction: the loader-wave kernels only, up to fixup_max slices, never in front of a fused GroupNorm
    {
        const Plan pl{256, 160, kPingPong, 4};
        CHECK(cfg.fixup_max == 4 && fixup_plan_ok(cfg, pl, 2048, 1280, 96ll << 20, false));
        CHECK(!fixup_plan_ok(cfg, pl, 2048, 1280, 96ll << 20, true) && !fixup_plan_ok(cfg, pl, 2048, 1280, 0, false));
        CHECK(!fixup_plan_ok(cfg, Plan{256, 160, kPingPong, 5}, 2048, 1280, 96ll << 20, false));
        CHECK(!fixup_plan_ok(cfg, Plan{128, 160, kRing, 4}, 2048, 1280, 96ll << 20, false));
        CHECK(!fixup_plan_ok(cfg, pl, 2048, 1280, fixup_bytes(pl, 2048, 1280) - 1, false));
        PlanConfig off = cfg;
        off.fixup_max = 0;
        CHECK(!fixup_plan_ok(off, pl, 2048, 1280, 96ll << 20, false));
    }

    // family predicates: what the literals used to decode
    CHECK(!even_tn(Plan{128, 160, kRing, 1}) && even_tn(Plan{128, 128, kRing, 1}) && even_tn(Plan{64, 64, kRing, 1}));
    CHECK(!even_tn(Plan{64, 64, 103, 1}) && even_tn(Plan{64, 128, 103, 1}) && even_tn(pp128) && !even_tn(pp160));
    CHECK(wave_owns_64_rows(pp160) && wave_owns_64_rows(Plan{128, 128, kLoaderConsumer, 1}) && !wave_owns_64_rows(Plan{64, 128, kLoaderConsumer, 1}));
    CHECK(!wave_owns_64_rows(Plan{128, 160, 123, 1}) && !wave_owns_64_rows(Plan{64, 64, kRing, 1}));

    // the sweep: the grid of the plan table plus the extremes of M and of the workspace, both families, both planners
    const int Ms[] = {64, 95, 96, 128, 255, 256, 512, 1024, 2048, 4096, 8192, 32768, 1 << 20, (1 << 30) + 1, 2147483647 - 255, 2147483647};
    const int Ns[] = {64, 96, 128, 160, 256, 320, 640, 1280, 2560, 5120, 10240};
    const int Ks[] = {64, 512, 1280, 1536, 5760, 10240, 23040};
    const int64_t Ws[] = {0, 64ll << 10, (96ll << 20) + kWsTail, 1ll << 40, 1ll << 62};
    long plans = 0;
    for (int family : {0, 1})
        for (int M : Ms)
            for (int N : Ns)
                for (int K : Ks)
                    for (int batch : {1, 8})
                        for (int64_t whole : Ws) {
                            cfg.family = family;
                            const int64_t ws = gmd_ws_usable_bytes(whole);
                            for (bool geglu : {false, true}) {
                                check_plan(cfg, make_plan(cfg, M, N, K, batch, ws, geglu, false), M, N, K, batch, ws);
                                const Plan f = f32_plan(M, N, K, batch, ws, geglu);
                                check_plan(cfg, f, M, N, K, batch, ws);
                                CHECK(f.pf == kRing && (!geglu || (f.ksplit == 1 && f.bn != 160)));
                                int o4[4];
                                CHECK(gmd_split_plan_info(GMD_F32SW, M, N, K, batch, whole, geglu, o4) == GMD_OK && o4[0] == f.bm && o4[1] == f.bn &&
                                      o4[2] == 0 && o4[3] == f.ksplit);
                                for (int mode : {-1, 1}) {
                                    PlanConfig lc = cfg;
                                    lc.split_lc_mode = mode;
                                    split_lc_fits(lc, f, M, N, K, batch);
                                }
                                plans += 2;
                            }
                            check_plan(cfg, make_plan(cfg, M, N, K, batch, ws, false, true), M, N, K, batch, ws);
                            f32_colstats_ok(M, N, K, batch, ws, 10);
                            f32_out_ok(M, N, K, true, ws);
                            f32_qkv_vt_ok(M, N, K, N / 3 * 2, 64, ws);
                            conv_plan_ksplit(cfg, GMD_F16, M, K / 9, N, ws);
                        }
    // forced plans go through the same arithmetic (GMD_TUNING=1 processes only)
    for (int pf : {9, 1, 2, 103, 143, 244, 283})
        for (int ks : {0, 2, 16}) {
            cfg.force = Force{128, 160, pf, ks};
            for (int M : Ms)
                for (int64_t whole : Ws) check_plan(cfg, make_plan(cfg, M, 1280, 5760, 1, gmd_ws_usable_bytes(whole), false), M, 1280, 5760, 1, gmd_ws_usable_bytes(whole));
        }
    // conv channel block at the largest tensors the entry points accept (< 4 GiB)
    for (int B : {1, 8, 64})
        for (int HW : {8, 64, 512, 2048})
            for (int Cin : {64, 640, 2560})
                for (int dtype : {GMD_F32, GMD_BF16, GMD_F32S}) {
                    const int c = conv_channel_block(PlanConfig{}, B, HW, HW, Cin, 320, dtype);
                    CHECK(c > 0 && c <= Cin && Cin % c == 0);
                }
    printf("%ld plans checked, %d failures\n", plans, failures);
    return failures ? 1 : 0;
}
