"""GPU: the refusing side of the column-statistics plan query.  Where gmd_gemm_colstats_plan answers 0, a launch that asks for
statistics is refused before anything is launched: GMD_ERR_UNSUPPORTED, the documented message, output and statistics untouched.  (The
accepting side -- statistics that are right -- is test_stats_handoff_gpu.py.)"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BUCKET = 10
UNSUPPORTED = 3  # GMD_ERR_UNSUPPORTED


def _launch(ops, lib, code, M, N, K, dtype, seed):
    """gmd_gemm_nt with statistics into NaN-filled buffers -> (status, output, statistics)"""
    g = torch.Generator().manual_seed(seed)
    a = torch.randn(M, K, generator=g).to("cuda", dtype)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to("cuda", dtype)
    out = torch.full((M, N), float("nan"), dtype=dtype, device="cuda")
    st = torch.full((M // 64, N // BUCKET, 2), float("nan"), dtype=torch.float32, device="cuda")
    ws = ops._workspace(a.device)
    rc = lib.gmd_gemm_nt(a.data_ptr(), w.data_ptr(), out.data_ptr(), code, ops.dtype_code(dtype), M, N, K, K, K, N, 1, 0, 0, M * N, None, None, 0, 0,
                         None, N, 0, 1.0, ops.ACT_NONE, st.data_ptr(), BUCKET, ws.data_ptr(), ops.WORKSPACE_BYTES, ops._stream())
    torch.cuda.synchronize()
    return rc, out, st, a, w


def _check_pair(ops, lib, code, dtype, accept, refuse, message):
    """accept / refuse: (M, N, K, plan family) on either side of the point where the query flips"""
    prev = lib.gmd_gemm_plan_family(-1)
    try:
        M, N, K, family = accept
        lib.gmd_gemm_plan_family(family)
        assert lib.gmd_gemm_colstats_plan(code, M, N, K, 1, ops.WORKSPACE_BYTES, BUCKET) == 1
        rc, out, st, a, w = _launch(ops, lib, code, M, N, K, dtype, 1)
        assert rc == 0, lib.gmd_last_error()
        assert bool(torch.isfinite(out.float()).all()) and bool(torch.isfinite(st).all())
        ref = a.float() @ w.float().t()
        assert float((out.float() - ref).abs().max()) <= 2.0 ** -7 * float(ref.abs().max()) + 1e-6  # (bf16 rounding of the output: 2^-9 relative)
        sums = out.float().view(M // 64, 64, N // BUCKET, BUCKET).sum(dim=(1, 3))
        assert torch.allclose(st[..., 0], sums, rtol=1e-4, atol=1e-2)

        M, N, K, family = refuse
        lib.gmd_gemm_plan_family(family)
        assert lib.gmd_gemm_colstats_plan(code, M, N, K, 1, ops.WORKSPACE_BYTES, BUCKET) == 0
        rc, out, st, _a, _w = _launch(ops, lib, code, M, N, K, dtype, 2)
        assert rc == UNSUPPORTED and message in lib.gmd_last_error().decode(), lib.gmd_last_error()
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(st).all()), "a refused launch wrote to its output or its statistics"
    finally:
        lib.gmd_gemm_plan_family(prev)


def test_colstats_refused_where_the_plan_query_says_no_bf16():
    """bf16 256 x 160 x 512: the co-running family takes one 256 x 160 ping-pong tile (statistics), the default family 64 x 64 tiles."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import GMD_BF16, lib

    _check_pair(ops, lib(), GMD_BF16, torch.bfloat16, (256, 160, 512, 1), (256, 160, 512, 0),
                "cannot emit column statistics (they need the full-tile row epilogue of an unsplit 128-row ring launch: ask gmd_gemm_colstats_plan first)")


def test_colstats_refused_where_the_plan_query_says_no_f32_split():
    """GMD_F32S plans do not depend on the family: its query flips with the tile count.  The smallest accepting shapes of
    tests/golden/gemm_plan_table.json are the 256-tile ones (M N = 5242880); along M at N = 1280 that is 4096 rows, and one row
    block fewer (248 tiles of 128 x 160) falls back to 64 x 64 tiles, which have no row epilogue."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import GMD_F32S, lib

    _check_pair(ops, lib(), GMD_F32S, torch.float32, (4096, 1280, 64, 0), (3968, 1280, 64, 0),
                "this float32 launch cannot emit column statistics (full-tile row epilogue of an unsplit 128-row launch: ask gmd_gemm_colstats_plan first)")
