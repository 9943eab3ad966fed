// Launch planning of the dense contractions (gmd_gemm_nt, gmd_gemm_qkv_vt, gmd_conv3x3): tile, kernel family, K slices, in-kernel
// reduction, tile order, conv channel block, and what a launch may fuse (GroupNorm statistics, transposed V, pre-split output).
// Host arithmetic only -- plain C++, no HIP -- shared by the 16-bit path (gemm.hip) and float32 on the matrix cores (gemm_split.hip),
// which keep the kernels and the dispatch from a finished Plan to an instantiation.  The planning functions are pure: they read the
// PlanConfig they are given and nothing else.
#pragma once
#include "../../include/gmd_hip.h"
#include "gemm_params.h"

void gmd_set_error(const char* fmt, ...);  // gmd_error.cpp

namespace gmd {

// Kernel families by their code in the C ABI (gmd_gemm_plan_info, gmd_gemm_plan_override, GMD_GEMM_FORCE)
enum Family : int {
    kRing = 0,              // default: two-stage LDS-DMA ring (128-row tiles) / 64x64 LDS-DMA tiles
    kRegStaged1 = 1,        // register-staged fallbacks (bfloat16, overrides only)
    kRegStaged2 = 2,
    kForceRing = 9,         // override only: "the default ring", since 0 means "keep the heuristic" there
    kRingVariant = 100,     // 1WS: ring kernels with S stages, W = 0 / 2 / 4 for 1 / 2 / 4 waves in M (bfloat16, overrides only)
    kLoaderConsumer = 244,  // gemm_lc_kernel: 128- / 64-row tiles, 4 consumer + 4 loader waves, one workgroup per CU
    kPingPong = 283,        // gemm_pp_kernel (and the conv patch kernels): 256-row tiles, 8 consumer + 4 loader waves
};
inline bool is_loader_wave(int pf) { return pf == kPingPong || pf == kLoaderConsumer; }  // the round-4 kernels, one workgroup per CU
inline bool is_ring_variant(int pf) { return pf >= kRingVariant && !is_loader_wave(pf); }
inline bool has_fixup(int pf) { return is_loader_wave(pf); }  // in-kernel split-K reduction (splitk_fixup of gemm.hip)

struct Plan {
    int bm, bn, pf, ksplit;
};
// every wave owns 64 rows x (BN/2) columns: the kernels whose row epilogue emits column statistics
inline bool wave_owns_64_rows(const Plan& pl) {
    return (pl.pf == kRing && pl.bm == 128) || (pl.pf == kPingPong && pl.bm == 256) || (pl.pf == kLoaderConsumer && pl.bm == 128);
}
// an even number of 16-column tiles per wave (GEGLU pairs value / gate tiles inside a wave): not TN = 5, not ring<1,4,1,.> (TN = 1)
inline bool even_tn(const Plan& pl) { return !(pl.bn == 160 || (is_ring_variant(pl.pf) && pl.bm == 64 && pl.bn == 64)); }

// GMD_GEMM_FORCE="bm,bn,pf,ksplit" / gmd_gemm_plan_override(): 0 = keep the heuristic
struct Force {
    int bm = 0, bn = 0, pf = 0, ks = 0;
};

// Every tuning knob of the planner.  Filled from the environment once, when the library is loaded (load_plan_config); the in-process
// setters of the C ABI write to the one process-wide instance; plan_config() hands a launch or a query its copy.
struct PlanConfig {
    Force force;          // GMD_GEMM_FORCE (GMD_TUNING=1 only), gmd_gemm_plan_override()
    bool pp_enabled;      // GMD_PP=0 keeps the round-3 plans (A/B measurements of whole runs)
    int family_pin;       // GMD_PP=b / GMD_PP=1 pin plan family 1 / 0 for the whole process; -1 = the calling thread's choice
    int family;           // plan family in force (see make_plan): the pin, else gmd_gemm_plan_family() of the calling thread
    int f1_target;        // GMD_F1_TARGET, GMD_F1_MIN_STEPS, GMD_F1_BN128: K slices / tile width of family 1 (see make_plan)
    int f1_min_steps;
    bool f1_bn128;
    int fixup_max;        // GMD_SPLITK_FIXUP, gmd_splitk_fixup_max(): in-kernel split-K reduction up to this many K slices (0 = off)
    int conv_patch_mode;  // GMD_CONV_PATCH, gmd_conv_patch_override(): see use_conv_patch
    int split_lc_mode;    // GMD_SPLIT_LC, gmd_gemm_plan_override(pf): see split_lc_fits
    int conv_cblk;        // GMD_CONV_CBLK (GMD_TUNING=1 only): channel block of the 16-bit convolutions, 0 = heuristic
};
PlanConfig load_plan_config();  // from the environment
PlanConfig plan_config();       // the process-wide configuration, `family` resolved for the calling thread

// ---- plans ----
Plan base_plan(int M, int N, int K, int batch, int64_t ws_bytes, bool pair_tiles, const Force& force);
Plan make_plan(const PlanConfig& cfg, int M, int N, int K, int batch, int64_t ws_bytes, bool pair_tiles, bool want_cs = false);
Plan f32_plan(int M, int N, int K, int batch, int64_t ws_bytes, bool geglu);
int64_t fixup_bytes(const Plan& pl, int M, int N);
bool fixup_plan_ok(const PlanConfig& cfg, const Plan& pl, int M, int N, int64_t ws_bytes, bool defer_reduce);
bool colstats_plan_ok(const PlanConfig& cfg, const Plan& pl, int M, int N, int batch, int bucket, int64_t ws_bytes);
bool qkv_vt_plan_ok(const Plan& pl, int M, int N, int batch, int vt_col0, int vt_tokens);
bool qkv_vt_ok(const PlanConfig& cfg, int dtype, int M, int N, int K, int vt_col0, int vt_tokens, int64_t ws_bytes);  // any dtype; usable bytes
const char* plan_unsupported(const PlanConfig& cfg, const Plan& pl, const GemmParams& p, int batch, int64_t ws_bytes);
int pick_tile_group(const Plan& pl, int M, int N, int K);

// ---- float32 on the matrix cores (ws_bytes: the USABLE bytes, without the counter tail) ----
bool f32_full_rows(const Plan& pl, int M, int N, int batch);
bool f32_colstats_ok(int M, int N, int K, int batch, int64_t ws_bytes, int bucket);
bool f32_out_ok(int M, int N, int K, bool geglu, int64_t ws_bytes);
bool f32_qkv_vt_ok(int M, int N, int K, int vt_col0, int vt_tokens, int64_t ws_bytes);
bool split_lc_fits(const PlanConfig& cfg, const Plan& pl, int M, int N, int K, int batch);

// ---- conv3x3 ----
int conv_channel_block(int B, int Hin, int Win, int Cin, int Cout, int elem_bytes, int step);
int conv_channel_block(const PlanConfig& cfg, int B, int Hin, int Win, int Cin, int Cout, int dtype);
bool conv_patch_ok(const GemmParams& p);
bool use_conv_patch(const PlanConfig& cfg, const Plan& pl, const GemmParams& p);
bool conv_out_shape(int Hin, int Win, int stride, int& upsample, int pad_mode, int& Hout, int& Wout, int& pad_lo);
int conv_plan_ksplit(const PlanConfig& cfg, int dtype, int64_t M, int Cin, int Cout, int64_t ws_bytes);

// ---- nearest-2x upsampling conv3x3 as four 2x2 phase convolutions (gmd_conv3x3_up2) ----
// The launch is planned as the GEMM it runs: M = 4 ceil(B Hin Win / 256) 256 rows (whole 256-row panels per phase), N = Cout,
// K = 4 Cin.  True (and `pl`, `M` filled) when that plan is the 256-row ping-pong kernel, the only one with a phase loader; K slices
// only where the in-kernel reduction takes them.  bucket > 0: the launch is to emit column statistics (false when it cannot).
bool up2_plan(const PlanConfig& cfg, int dtype, int B, int Hin, int Win, int Cin, int Cout, int bucket, int64_t ws_bytes, Plan& pl, int& M);

inline bool is_half(int dtype) { return dtype == GMD_BF16 || dtype == GMD_F16; }
inline bool is_split(int dtype) { return dtype == GMD_F32S || dtype == GMD_F32SW || dtype == GMD_F32SA; }

}  // namespace gmd
