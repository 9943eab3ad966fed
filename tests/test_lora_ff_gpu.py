"""GPU: LoRA on the feed-forward and proj_in / proj_out (``targets="transformer"``).  The fused update + GEGLU launch
(gmd_lora_geglu) per element against float64 and the derived bound of tests/lora_ff_ref.py; its write footprint, row independence,
the device-resident scale, the composed route; the adapted UNet against the merged oracle in every dtype mode; the launches of an
adapted block; the pipelines against the CPU loop run with the merged oracle UNet."""
import functools

import pytest
import torch

import lora_ff_ref as FR
import lora_ref as R
import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
MODEL_TOL = {F32: 2e-5, BF16: 3e-2, F16: 4e-3}  # tests/test_models_gpu.py and test_unet_with_adapter_against_the_merged_oracle
CANARY = 1234.0  # exactly representable in both 16-bit types; nothing the launches produce


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rms(a, b):
    return float(((a.double().cpu() - b.double().cpu()) ** 2).mean().sqrt())


def _pad(n, m):
    return (n + m - 1) // m * m


def _scales(value, idx, n=7):
    """A device table with ``value`` at ``idx`` and a value that would be noticed (1e4) everywhere else."""
    s = torch.full((n,), 1.0e4, dtype=torch.float32)
    s[idx] = value
    return s.to(DEV)


def _operands(M, C, rank, dtype, seed):
    """x [M, C], the factors zero-padded to a multiple of 32 (b [8C, Rp], rows already in the interleaved order: for the kernel any
    row order is just a matrix), y0 [M, 8C] in the interleaved layout (CPU, values of ``dtype``)."""
    g = torch.Generator().manual_seed(seed)
    rp = _pad(rank, 32)
    x = torch.randn(M, C, generator=g).to(dtype)
    a, b = torch.zeros(rp, C), torch.zeros(8 * C, rp)
    a[:rank] = torch.randn(rank, C, generator=g) / C ** 0.5
    b[:, :rank] = torch.randn(8 * C, rank, generator=g) / rank ** 0.5
    y0 = torch.randn(M, 8 * C, generator=g).to(dtype)
    return x, a.to(dtype), b.to(dtype), y0


def _launch(x, a, b, y0, sc, idx, ldy=None, ldf=None, extra_rows=0):
    """gmd_lora_geglu through the C ABI with y0 in a canary-filled [M, ldy] buffer and F in a canary-filled [M + extra_rows, ldf] one.
    Returns (F buffer, X after, Y buffer after, Y buffer before), on the CPU."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import check, lib

    M, C = x.shape
    ldy, ldf = ldy or 8 * C, ldf or 4 * C
    ybuf = torch.full((M, ldy), CANARY, dtype=y0.dtype)
    ybuf[:, :8 * C] = y0
    dx, da, db, dy = x.to(DEV), a.to(DEV), b.to(DEV), ybuf.to(DEV)
    f = torch.full((M + extra_rows, ldf), CANARY, dtype=y0.dtype, device=DEV)
    check(lib().gmd_lora_geglu(dx.data_ptr(), da.data_ptr(), db.data_ptr(), dy.data_ptr(), f.data_ptr(), ops.dtype_code(x.dtype), M, C,
                               a.shape[0], C, ldy, ldf, sc.data_ptr(), idx, torch.cuda.current_stream().cuda_stream), "gmd_lora_geglu")
    torch.cuda.synchronize()
    return f.cpu(), dx.cpu(), dy.cpu(), ybuf


def _tiles_per_workgroup(row_blocks, C):
    """64-column tiles of Y one workgroup walks: the host's split of csrc/lora.hip restated -- the 8C / 64 tiles are split over
    gridDim.y only as far as ceil(512 / row blocks)."""
    ntiles = 8 * C // 64
    nsplit = max(1, min(ntiles, -(-512 // row_blocks)))
    return -(-ntiles // nsplit)


# ---------------------------------------------------------------------------------------------------------------------------
# kernel, per element
# ---------------------------------------------------------------------------------------------------------------------------
CS, MS, RANKS = (64, 128), (1, 63, 64, 65, 130, 257), (4, 33, 128)  # rank 33 is padded to 64


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("C", CS)
def test_kernel_per_element_zero_violations(dtype, C):
    """C x M x rank, the full product; every launch here has gridDim.y > 1 (few row blocks: one tile per workgroup); scales
    0.7 / -1.3 and the index alternate."""
    worst, c = 0.0, 0
    for M in MS:
        assert _tiles_per_workgroup(_pad(M, 64) // 64, C) == 1 and 8 * C // 64 > 1  # gridDim.y = 8C / 64 > 1
        for rank in RANKS:
            s, idx = (0.7, -1.3)[c % 2], (0, 5)[(c // 2) % 2]
            x, a, b, y0 = _operands(M, C, rank, dtype, seed=100 + 40 * C + c)
            assert a.shape[0] == {4: 32, 33: 64, 128: 128}[rank]
            f, _, _, _ = _launch(x, a, b, y0, _scales(s, idx), idx)
            ref, bound = FR.geglu_update_ref_bound(x, a, b, y0, torch.tensor(s, dtype=F32), dtype)
            worst = max(worst, P.assert_elementwise(f, ref, bound, f"lora_geglu {dtype} M={M} C={C} r={rank} idx={idx}", tile=(16, 32)))
            c += 1
    print(f"lora_geglu {dtype} C={C}: {c} cases, max |err| / bound = {worst:.3f}")


# (M, C, rank): 130 row blocks -> 4 splits of 2 tiles; 259 row blocks -> 2 splits of 4 tiles; 514 row blocks -> gridDim.y = 1, all
# 8 tiles in one workgroup: the Bw tile prefetched under the MFMAs of the tile before, the stage reused tile after tile
MULTI_TILE = ((8259, 64, 8, 2), (16515, 64, 33, 4), (32833, 64, 4, 8))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_kernel_several_tiles_per_workgroup(dtype):
    for c, (M, C, rank, tiles) in enumerate(MULTI_TILE):
        assert _tiles_per_workgroup(_pad(M, 64) // 64, C) == tiles
        x, a, b, y0 = _operands(M, C, rank, dtype, seed=700 + c)
        f, _, _, _ = _launch(x, a, b, y0, _scales(0.7, 5), 5, ldf=4 * C + 8)
        ref, bound = FR.geglu_update_ref_bound(x, a, b, y0, torch.tensor(0.7, dtype=F32), dtype)
        P.assert_elementwise(f[:, :4 * C], ref, bound, f"lora_geglu {dtype} M={M} C={C} r={rank}, {tiles} tiles per workgroup", tile=(16, 32))
        assert bool((f[:, 4 * C:] == CANARY).all())


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_write_footprint_and_read_only_inputs(dtype):
    """F inside a canary-filled buffer (columns [4C, ldf) and the rows from M on keep their bits, every element of the target is
    written: a GEGLU output equal to the canary does not occur); X and Y -- Y's pad columns included -- are bit-unchanged."""
    M, C, rank = 161, 128, 8
    x, a, b, y0 = _operands(M, C, rank, dtype, seed=9)
    f, x_after, y_after, y_before = _launch(x, a, b, y0, _scales(1.0, 0), 0, ldy=8 * C + 24, ldf=4 * C + 40, extra_rows=70)
    assert bool((f[M:] == CANARY).all()) and bool((f[:M, 4 * C:] == CANARY).all())
    assert not bool((f[:M, :4 * C] == CANARY).any())
    assert torch.equal(x_after.view(torch.int16), x.view(torch.int16))
    assert torch.equal(y_after.view(torch.int16), y_before.view(torch.int16))
    ref, bound = FR.geglu_update_ref_bound(x, a, b, y0, torch.tensor(1.0, dtype=F32), dtype)
    P.assert_elementwise(f[:M, :4 * C], ref, bound, f"lora_geglu {dtype} in padded buffers")


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_row_independence_and_a_zero_scale(dtype):
    """A row's bits depend neither on M nor on the other rows, ACROSS DIFFERENT GRIDS: the first 64 rows of an M = 257 launch (5 row
    blocks x 8 splits) and of an M = 8259 launch (130 x 4, two tiles per workgroup) against an M = 64 launch of those rows, and with
    every OTHER row replaced.  scales[index] = 0 gives exactly the GEGLU of Y: the bits of gmd_geglu_interleaved, whatever the
    factors."""
    from gm_diffusion import hip_ops as ops

    C, rank = 64, 16
    sc = _scales(0.9, 5)
    for M in (257, 8259):
        x, a, b, y0 = _operands(M, C, rank, dtype, seed=21 + M)
        big = _launch(x, a, b, y0, sc, 5)[0]
        small = _launch(x[:64].contiguous(), a, b, y0[:64].contiguous(), sc, 5)[0]
        assert torch.equal(big[:64].view(torch.int16), small.view(torch.int16))
        x2, y2 = x.clone(), y0.clone()
        x2[64:], y2[64:] = -x[64:] * 3, y0[64:] + 1
        other = _launch(x2, a, b, y2, sc, 5)[0]
        assert torch.equal(other[:64].view(torch.int16), small.view(torch.int16)) and not torch.equal(other[64:], big[64:])
    assert _tiles_per_workgroup(5, C) == 1 and _tiles_per_workgroup(130, C) == 2 and _tiles_per_workgroup(1, C) == 1
    x, a, b, y0 = _operands(257, C, rank, dtype, seed=25)
    zero = _launch(x, a, b, y0, _scales(0.0, 5), 5)[0]
    plain = ops.geglu_interleaved(y0.to(DEV)).cpu()
    assert torch.equal(zero.view(torch.int16), plain.view(torch.int16))
    _, a2, b2, _ = _operands(257, C, 128, dtype, seed=26)
    assert torch.equal(_launch(x, a2, b2, y0, _scales(0.0, 5), 5)[0].view(torch.int16), zero.view(torch.int16))
    v, g = FR.deinterleave_cols(y0.double())
    assert rel_err(zero, v * torch.nn.functional.gelu(g)) < 2 * P.unit_roundoff(dtype)
    assert not torch.equal(zero, _launch(x, a, b, y0, sc, 5)[0])


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_one_graph_serves_every_scale(dtype):
    from gm_diffusion import hip_ops as ops

    M, C, rank = 161, 64, 8
    x, a, b, y0 = _operands(M, C, rank, dtype, seed=31)
    dx, da, db, dy = (t.to(DEV) for t in (x, a, b, y0))
    sc = torch.zeros(7, dtype=F32, device=DEV)
    sc[5] = 0.5
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.lora_geglu(dx, da, db, dy, sc, 5, fused=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        f = ops.lora_geglu(dx, da, db, dy, sc, 5, fused=True)
    for s in (0.5, -1.25, 0.0):
        sc[5] = s
        g.replay()
        torch.cuda.synchronize()
        ref, bound = FR.geglu_update_ref_bound(x, a, b, y0, torch.tensor(s, dtype=F32), dtype)
        P.assert_elementwise(f.cpu(), ref, bound, f"replay at scale {s} {dtype}")
    assert torch.equal(dy.cpu(), y0)  # Y is read-only: three replays later it still holds the pre-activation


def test_argument_checks_and_empty_launches():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import HipExtensionError, lib

    buf = torch.zeros(1 << 16, dtype=BF16, device=DEV)
    p, es = buf.data_ptr(), 2
    # X [8, 64] at 0, Aw [32, 64] at 4096, Bw [512, 32] at 8192, Y [8, 512] at 32768, F [8, 256] at 40960 (elements)
    X, A, B_, Y, F_ = p, p + 4096 * es, p + 8192 * es, p + 32768 * es, p + 40960 * es
    sc = _scales(1.0, 0)
    n = lib().gmd_lora_geglu

    def args(**o):
        return [o.get("X", X), A, B_, o.get("Y", Y), o.get("F", F_), o.get("dtype", 1), o.get("M", 8), o.get("C", 64), o.get("Rp", 32),
                o.get("ldx", 64), o.get("ldy", 512), o.get("ldf", 256), o.get("sc", sc.data_ptr()), o.get("idx", 0), None]

    assert n(*args()) == 0
    assert n(*args(M=0)) == 0 and n(*args(M=0, X=None, Y=None, F=None)) == 0   # an empty launch
    assert n(*args(M=-1)) == 1
    assert n(*args(C=96, ldx=96, ldy=768, ldf=384)) == 1 and n(*args(C=32, ldx=32)) == 1   # C % 64
    assert n(*args(Rp=16)) == 1 and n(*args(Rp=48)) == 1                      # Rp % 32
    assert n(*args(Rp=160)) == 1                                              # rank above 128
    assert n(*args(sc=None)) == 1 and n(*args(idx=-1)) == 1
    assert n(*args(X=X + 2)) == 1 and n(*args(Y=Y + 2)) == 1 and n(*args(F=F_ + 2)) == 1   # alignment
    assert n(*args(ldy=504)) == 1 and n(*args(ldy=516)) == 1                  # ldy < 8C, ldy % 8
    assert n(*args(ldf=248)) == 1 and n(*args(ldf=260)) == 1                  # ldf < 4C, ldf % 8
    assert n(*args(ldx=56)) == 1 and n(*args(ldx=68)) == 1
    assert n(*args(F=X)) == 1 and n(*args(F=X + 64 * es)) == 1                # F overlaps X
    assert n(*args(F=Y)) == 1 and n(*args(F=Y + 8 * 512 * es - 16)) == 1      # F overlaps Y
    assert n(*args(X=None)) == 1 and n(*args(F=None)) == 1
    assert n(*args(dtype=0)) == 3 and n(*args(dtype=3)) == 3                  # float32 / split dtypes are composed by the caller
    err = lib().gmd_last_error()
    assert b"gmd_lora_geglu" in err and b"gmd_gemm_nt" in err and b"gmd_scaled_add" in err and b"gmd_geglu" in err
    torch.cuda.synchronize()
    x, a, b, y = buf[:512].view(8, 64), buf[4096:4096 + 2048].view(32, 64), buf[8192:8192 + 16384].view(512, 32), buf[32768:32768 + 4096].view(8, 512)
    assert ops.lora_geglu(x, a, b, y, sc, 0).shape == (8, 256)
    with pytest.raises(HipExtensionError):
        ops.lora_geglu(x, a, b, torch.zeros(8, 512, dtype=F16, device=DEV), sc, 0)      # dtype mismatch
    with pytest.raises(HipExtensionError):
        ops.lora_geglu(x, a, b[:256], y, sc, 0)                                           # b is not [8C, Rp]
    with pytest.raises(HipExtensionError):
        ops.lora_geglu(x, a, b, y, sc, 7)                                                 # index outside the table
    assert ops.lora_geglu(x[:0], a, b, y[:0], sc, 0).shape == (0, 256)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_fused_and_composed_routes_agree(dtype):
    from gm_diffusion import hip_ops as ops

    M, C, rank = 257, 128, 33
    x, a, b, y0 = _operands(M, C, rank, dtype, seed=41)
    sc = _scales(0.6, 2)
    dx, da, db = x.to(DEV), a.to(DEV), b.to(DEV)
    yf, yc = y0.to(DEV), y0.to(DEV)
    f = ops.lora_geglu(dx, da, db, yf, sc, 2, fused=True).cpu()
    c = ops.lora_geglu(dx, da, db, yc, sc, 2, fused=False).cpu()
    torch.cuda.synchronize()
    assert torch.equal(yf.cpu(), y0) and not torch.equal(yc.cpu(), y0)  # the composed route updates y in place, the fused one reads it
    s = torch.tensor(0.6, dtype=F32)
    ref, b_f = FR.geglu_update_ref_bound(x, a, b, y0, s, dtype)
    _, b_c = FR.geglu_update_ref_bound(x, a, b, y0, s, dtype, route="composed")
    P.assert_elementwise(f, ref, b_f, f"fused {dtype}")
    P.assert_elementwise(c, ref, b_c, f"composed {dtype}")
    P.assert_elementwise(f, c.double(), b_f + b_c, f"fused vs composed {dtype}")


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_geglu_interleaved_equals_geglu_over_halves(dtype):
    """The composed route's second launch: the same bits as gmd_geglu on the de-interleaved tensor (one device function, one rounding)."""
    from gm_diffusion import hip_ops as ops

    g = torch.Generator().manual_seed(7)
    for M, F_ in ((1, 16), (67, 256), (130, 1280)):
        y = (3 * torch.randn(M, 2 * F_, generator=g)).to(dtype)
        v, gate = FR.deinterleave_cols(y)
        got = ops.geglu_interleaved(y.to(DEV)).cpu()
        want = ops.geglu(torch.cat([v, gate], 1).contiguous().to(DEV)).cpu()
        assert got.shape == (M, F_) and torch.equal(got, want)
        assert rel_err(got, v.double() * torch.nn.functional.gelu(gate.double())) < 2 * P.unit_roundoff(dtype)


# ---------------------------------------------------------------------------------------------------------------------------
# UNet (tiny config, 16 x 16 latents, batch 2)
# ---------------------------------------------------------------------------------------------------------------------------
RANK, SEED, ALPHA = 4, 11, 2.0
# (families, gain).  The gains come from the float32 ORACLE and from torch's own bfloat16 arithmetic on the CPU, not from the HIP model:
#   * all twelve targets at the gain 2 of tests/test_lora_gpu.py make every adapted weight ~1.7x its base weight; the merged oracle
#     evaluated by torch in bfloat16 on the CPU is then 6.6e-2 (hooked: 6.1e-2) off its own float32 result -- twice the bfloat16 gate
#     of 3e-2, which no bfloat16 implementation of that model can meet.  At gain 1 the same figure is 1.3e-2 (the oracle without an
#     adapter: 1.1e-2) and the adapter still moves the float32 output by 0.91 of its norm (the attention-only adapter at gain 2: 0.69);
#   * ff.net.2 alone moves the output by 0.31 at gain 2, too close to 10 x the bfloat16 gate: gain 4 (0.55); proj_out alone: 0.95.
ADAPTERS = {"all": (None, 1.0), "ff2": (("ff2",), 4.0), "proj_out": (("proj_out",), 2.0)}

@functools.lru_cache(maxsize=None)
def _refs():
    from oracle import fixtures

    return fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8)


@functools.lru_cache(maxsize=None)
def _adapter(which):
    """(canonical factors, kohya state dict with 4-D factors for the 1x1-convolution proj_in / proj_out) of the SDR oracle UNet."""
    ou, _ = _refs()
    families, gain = ADAPTERS[which]
    canon = FR.canonical(ou, RANK, SEED, gain, alpha=ALPHA, families=families)
    return canon, FR.to_convention(canon, "kohya", conv_names=FR.conv_targets(ou))


def _hip_unet(ou, dtype):
    from gm_diffusion.components import UNet2DConditionModel

    m = UNet2DConditionModel(**vars(ou.config))
    m.load_state_dict(ou.state_dict())
    return m.to(DEV, dtype)


@functools.lru_cache(maxsize=None)
def _unet_inputs():
    g = torch.Generator().manual_seed(61)
    return torch.randn(1, 4, 16, 16, generator=g), torch.randn(2, 77, 64, generator=g)


@functools.lru_cache(maxsize=None)
def _unet_case(which):
    """The CPU references, computed once per adapter: [negative; positive] rows of one latent pair (so cfg_shared applies)."""
    ou, _ = _refs()
    canon, _ = _adapter(which)
    lat, ctx = _unet_inputs()
    x = torch.cat([lat, lat])
    with torch.no_grad():
        eps = {s: FR.merged_oracle(ou, canon, s)(x, torch.tensor(501), encoder_hidden_states=ctx)[0] for s in (1.0, 0.5)}
        plain = ou(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
    return eps, plain


@pytest.mark.parametrize("which", sorted(ADAPTERS))
@pytest.mark.parametrize("dtype,mode", [(F32, "split"), (F32, "exact"), (BF16, "split"), (F16, "split")])
def test_unet_with_the_wider_adapter_against_the_merged_oracle(dtype, mode, which):
    """The twelve-target adapter, and the adapters with only ff.net.2 (the ACT_GEGLU branch of the two-GEMM route) and only proj_out (the
    colstats branch), at the gates of test_unet_with_adapter_against_the_merged_oracle."""
    from gm_diffusion import hip_ops as ops

    prev = ops.set_f32_mode(mode)
    try:
        ou, _ = _refs()
        _, sd = _adapter(which)
        lat, ctx = _unet_inputs()
        eps, plain = _unet_case(which)
        tol = MODEL_TOL[dtype]
        hu, never = _hip_unet(ou, dtype), _hip_unet(ou, dtype)
        dlat, dctx = lat.to(DEV), ctx.to(DEV)
        dx = torch.cat([dlat, dlat])
        base = never(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        hu.load_lora(sd, targets="transformer")
        got = hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        e = rel_err(got, eps[1.0])
        print(f"UNet + LoRA[{which}] {dtype} {mode}: rel err vs the merged oracle {e:.3e} (tol {tol:.0e}); the adapter moves the output by "
              f"{rel_err(got, base):.3f}")
        assert got.shape == eps[1.0].shape and e < tol, e
        assert rel_err(got, base) > 10 * tol and rel_err(eps[1.0], plain) > 10 * tol
        # packed: eager == graph replay == cfg_shared, bit for bit
        c = hu.prepare_context(dctx)
        hu.set_timestep(501)
        full = hu.forward_packed(hu.pack_input(dlat, dup=2), 2, 16, 16, c)
        assert torch.equal(full, got)
        shared = hu.forward_packed(hu.pack_input(dlat, dup=1), 2, 16, 16, c, cfg_shared=True)
        assert torch.equal(shared, full)
        gph = hu.graphed_forward(2, 16, 16, c, cfg_shared=True)
        hu.pack_input(dlat, dup=1, out=gph.x)
        assert torch.equal(gph.replay(), full)
        # another scale through the SAME graph equals a fresh model at that scale, and the merged oracle at that scale
        n_graphs = len(hu._graphs)
        hu.set_lora_scale(0.5)
        assert hu.graphed_forward(2, 16, 16, c, cfg_shared=True) is gph and len(hu._graphs) == n_graphs
        half = gph.replay().clone()
        fresh = _hip_unet(ou, dtype)
        fresh.load_lora(sd, targets="transformer")
        fresh.set_lora_scale(0.5)
        assert torch.equal(half, fresh(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0])
        assert rel_err(half, eps[0.5]) < tol and not torch.equal(half, full)
        hu.set_lora_scale(0.0)
        assert hu.graphed_forward(2, 16, 16, c, cfg_shared=True) is gph  # (refreshes the cached cross-attention K / V^T)
        assert rel_err(gph.replay(), base) < tol
        # unloaded: bit-identical to a UNet that never had an adapter, the adapter's graphs gone; reloaded: the same bits as before
        hu.unload_lora()
        assert not hu.has_lora and not any(("lora" in str(k)) for k in hu._graphs)
        assert torch.equal(hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0], base)
        hu.load_lora(sd, targets="transformer")
        c = hu.prepare_context(dctx)
        g2 = hu.graphed_forward(2, 16, 16, c, cfg_shared=True)
        assert g2 is not gph
        hu.pack_input(dlat, dup=1, out=g2.x)
        assert torch.equal(g2.replay(), full)
    finally:
        ops.set_f32_mode(prev)


def test_launches_of_plain_attention_only_and_feed_forward_adapted_blocks():
    """The launches per forward, counted at the hip_ops entry points, with ff_fused_ok forced on (the tiny UNet's C = 64 never takes
    ff_geglu_fused by itself; a stand-in built from the real GEMMs records the call).  No adapter and an attention-only adapter:
    ff_geglu_fused in every block, not one lora_geglu, the same GEMMs.  All twelve targets: no ff_geglu_fused; per block, in this
    order, gemm_nt (plain, [tokens, 8C]) -> lora_geglu -> gemm_nt (residual) -> lora_update (K = 4C); 11 lora_update per transformer
    and forward (8 attention, 2 of them only inside _cross_kv, + ff.net.2 + proj_in + proj_out)."""
    from gm_diffusion import hip_ops as ops

    ou, _ = _refs()
    lat, ctx = _unet_inputs()
    dx, dctx = torch.cat([lat, lat]).to(DEV), ctx.to(DEV)
    log = []
    names = ("gemm_nt", "lora_update", "lora_geglu", "geglu_interleaved", "ff_geglu_fused", "ff_fused_ok")
    real = {n: getattr(ops, n) for n in names}

    def wrap(name):
        def f(*a, **k):
            log.append((name, a, k))
            return real[name](*a, **k)
        return f

    def ff_stand_in(x, w1i, b1i, w2, b2, residual):
        log.append(("ff_geglu_fused", (), {}))
        return real["gemm_nt"](real["gemm_nt"](x, w1i, bias=b1i, act=ops.ACT_GEGLU), w2, bias=b2, residual=residual)

    def count(name):
        return sum(1 for e in log if e[0] == name)

    def run(hu):
        del log[:]
        c = hu.prepare_context(dctx)
        hu.set_timestep(501)
        hu.update_context(c)
        out = hu.forward_packed(hu.pack_input(dx), 2, 16, 16, c)
        return out, {n: count(n) for n in names}

    try:
        for n in ("gemm_nt", "lora_update", "lora_geglu", "geglu_interleaved"):
            setattr(ops, n, wrap(n))
        ops.ff_geglu_fused, ops.ff_fused_ok = ff_stand_in, (lambda *a, **k: True)
        hu = _hip_unet(ou, BF16)
        base, n0 = run(hu)
        assert n0["ff_geglu_fused"] == 16 and n0["lora_update"] == 0 and n0["lora_geglu"] == 0
        att = R.canonical(ou, RANK, SEED, 2.0, alpha=ALPHA)
        hu.load_lora(R.to_convention(att, "kohya"))
        _, n1 = run(hu)
        assert n1["ff_geglu_fused"] == 16 and n1["lora_update"] == 8 * 16 and n1["lora_geglu"] == 0 and n1["gemm_nt"] == n0["gemm_nt"]
        hu.unload_lora()
        hu.load_lora(R.to_convention(att, "kohya"), targets="transformer")  # the same adapter under the wider setting: the same launches
        _, n1t = run(hu)
        assert n1t == n1
        hu.unload_lora()
        hu.load_lora(_adapter("all")[1], targets="transformer")
        _, n2 = run(hu)
        assert n2["ff_geglu_fused"] == 0 and n2["lora_geglu"] == 16 and n2["lora_update"] == 11 * 16 and n2["geglu_interleaved"] == 0
        assert n2["gemm_nt"] == n0["gemm_nt"] + 2 * 16  # the two GEMMs of each feed-forward, nothing else
        seq = [e for e in log if e[0] in ("gemm_nt", "lora_update", "lora_geglu", "ff_geglu_fused")]
        at = [i for i, e in enumerate(seq) if e[0] == "lora_geglu"]
        assert len(at) == 16
        for i in at:
            C = seq[i][1][0].shape[1]
            g1, g2, up = seq[i - 1], seq[i + 1], seq[i + 2]
            assert g1[0] == "gemm_nt" and g1[1][1].shape == (8 * C, C) and g1[2].get("act", ops.ACT_NONE) == ops.ACT_NONE and "residual" not in g1[2]
            assert seq[i][1][3].shape[1] == 8 * C                       # lora_geglu reads that GEMM's [tokens, 8C] output
            assert g2[0] == "gemm_nt" and g2[1][1].shape == (C, 4 * C) and g2[2].get("residual") is not None
            assert up[0] == "lora_update" and up[1][0].shape[1] == 4 * C and up[1][3] is not None
        hu.unload_lora()
        hu.load_lora(_adapter("ff2")[1], targets="transformer")
        _, n3 = run(hu)
        assert n3["ff_geglu_fused"] == 0 and n3["lora_geglu"] == 0 and n3["lora_update"] == 16 and n3["gemm_nt"] == n0["gemm_nt"] + 2 * 16
        hu.unload_lora()
        again, n4 = run(hu)
        assert n4 == n0 and torch.equal(again, base)
    finally:
        for n in names:
            setattr(ops, n, real[n])


# ---------------------------------------------------------------------------------------------------------------------------
# pipelines (dual tiny, 2 prompts, 4 PNDM steps, 64 x 64)
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = 4


def _pndm():
    from gm_diffusion.components import PNDMScheduler

    return PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True, steps_offset=1,
                         set_alpha_to_one=False)


def _pipe(dtype, controlnet=None):
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    ou, og = _refs()
    pipe = StableDiffusionDualUNetPipeline(vae=None, text_encoder=None, tokenizer=None, unet=_hip_unet(ou, dtype), gm_unet=_hip_unet(og, dtype),
                                           scheduler=_pndm(), safety_checker=None, feature_extractor=None, requires_safety_checker=False,
                                           controlnet=controlnet)
    pipe.set_progress_bar_config(disable=True)
    pipe.load_lora_weights(_adapter("all")[1], targets="transformer")
    return pipe


def _kw(**extra):
    from oracle import fixtures

    pos, neg, lat = fixtures.make_inputs(2, 8, 8, cross_dim=64)
    return dict(prompt_embeds=pos.to(DEV), negative_prompt_embeds=neg.to(DEV), latents=lat.to(DEV), height=64, width=64,
                num_inference_steps=STEPS, guidance_scale=7.5, output_type="latent", **extra)


@functools.lru_cache(maxsize=None)
def _ref_loop(scale=1.0):
    from oracle import fixtures, pipelines as OP, schedulers as osched

    ou, og = _refs()
    pos, neg, lat = fixtures.make_inputs(2, 8, 8, cross_dim=64)
    unet = ou if scale is None else FR.merged_oracle(ou, _adapter("all")[0], scale)
    return OP.dual_loop(unet, og, osched.PNDMScheduler(), pos, neg, lat, num_inference_steps=STEPS, guidance_scale=7.5)


@pytest.mark.parametrize("mode", ["split", "exact"])
def test_pipeline_f32_against_the_cpu_loop_with_the_merged_oracle(mode):
    from gm_diffusion import hip_ops as ops

    prev = ops.set_f32_mode(mode)
    try:
        pipe = _pipe(F32)
        assert pipe.unet.has_lora and len(pipe.unet._lora_raw) == 12 * 16 and not pipe.gm_unet.has_lora
        sdr, gm = pipe(**_kw())
        ref_sdr, ref_gm = _ref_loop()
        e_sdr, e_gm = rms(sdr, ref_sdr), rms(gm, ref_gm)
        print(f"LoRA[transformer] pipeline float32 {mode}: latent RMS vs the CPU loop sdr={e_sdr:.3e} gm={e_gm:.3e}")
        assert e_sdr <= 1e-3 and e_gm <= 1e-3  # RMS_TOL of tests/test_pipeline_gpu.py
        plain_sdr, _ = _ref_loop(scale=None)
        assert rms(ref_sdr, plain_sdr) > 1e-2  # the adapter moves the result by far more than the gate
        sdr5, gm5 = pipe(**_kw(cross_attention_kwargs={"scale": 0.5}))
        r5 = _ref_loop(scale=0.5)
        assert rms(sdr5, r5[0]) <= 1e-3 and rms(gm5, r5[1]) <= 1e-3 and rms(r5[0], ref_sdr) > 1e-2
    finally:
        ops.set_f32_mode(prev)


def test_pipeline_graphs_and_streams_equal_eager_and_the_scale_kwarg_equals_set_lora_scale():
    pipe = _pipe(BF16)
    pipe.co_run_plans = True  # one plan family for every mode
    pipe.use_hip_graphs, pipe.overlap_streams = False, False
    a = pipe(**_kw())
    pipe.use_hip_graphs, pipe.overlap_streams = True, True
    b = pipe(**_kw())
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    counts = (len(pipe.unet._graphs), len(pipe.gm_unet._graphs))
    c = pipe(**_kw(cross_attention_kwargs={"scale": 0.5}))
    torch.cuda.synchronize()
    assert (len(pipe.unet._graphs), len(pipe.gm_unet._graphs)) == counts  # no new capture
    assert not torch.equal(c[0], b[0])
    again = pipe(**_kw())  # back at the UNet's own scale, through the same graphs
    torch.cuda.synchronize()
    assert torch.equal(again[0], b[0]) and torch.equal(again[1], b[1]) and pipe.unet._lora_scale == 1.0
    other = _pipe(BF16)
    other.co_run_plans = True
    other.unet.set_lora_scale(0.5)
    d = other(**_kw())
    torch.cuda.synchronize()
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])
    # the wider adapter is another model than its attention part alone (what ignore_unsupported leaves of it under the default)
    import warnings

    thin = _pipe(BF16)
    thin.unload_lora_weights()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        thin.load_lora_weights(_adapter("all")[1], ignore_unsupported=True)
    assert len(thin.unet._lora_raw) == 8 * 16
    thin.co_run_plans = True
    t = thin(**_kw())
    assert rms(t[0], b[0]) > 1e-2


def test_pipeline_lora_ip_adapter_and_controlnet_together():
    import controlnet_ref as CR
    import ip_adapter_ref as IR
    from gm_diffusion.components import ControlNetModel
    from oracle import unet as OU

    torch.manual_seed(5)
    cn_ref = CR.ControlNetRef(**CR.tiny_controlnet_config()).eval().requires_grad_(False)
    cn = ControlNetModel(**CR.tiny_controlnet_config())
    cn.load_state_dict(cn_ref.state_dict())
    pipe = _pipe(BF16, controlnet=cn.to(DEV, BF16))
    pipe.load_ip_adapter(IR.make_state_dict(OU.tiny_unet_config(4), tokens=4, clip_dim=32, seed=7, gain=2.0))
    g = torch.Generator().manual_seed(8)
    cimg = torch.rand(1, 3, 64, 64, generator=g).to(DEV)
    img = torch.randn(1, 1, 32, generator=g)
    emb = [torch.cat([torch.zeros_like(img), img]).to(DEV)]
    all3 = pipe(**_kw(control_image=cimg, ip_adapter_image_embeds=emb))
    no_lora = pipe(**_kw(control_image=cimg, ip_adapter_image_embeds=emb, cross_attention_kwargs={"scale": 0.0}))
    assert pipe.unet._lora_scale == 1.0  # the per-call scale is gone with its call
    no_ip = pipe(**_kw(control_image=cimg))
    no_cn = pipe(**_kw(control_image=cimg, ip_adapter_image_embeds=emb, controlnet_conditioning_scale=0.0))
    torch.cuda.synchronize()
    for other in (no_lora, no_ip, no_cn):
        assert rms(all3[0], other[0]) > 1e-2


def test_gm_pipeline_loads_the_wider_adapter():
    from gm_diffusion.pipelines import StableDiffusionGMPipeline
    from oracle import fixtures

    _, og = _refs()
    pipe = StableDiffusionGMPipeline(vae=None, text_encoder=None, tokenizer=None, unet=_hip_unet(og, BF16), scheduler=_pndm(),
                                     safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pos, neg, lat = fixtures.make_inputs(1, 8, 8, cross_dim=64)
    sdr_latent = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    kw = dict(prompt_embeds=pos.to(DEV), negative_prompt_embeds=neg.to(DEV), latents=lat.to(DEV), num_inference_steps=STEPS,
              guidance_scale=7.5, output_type="latent")
    plain = pipe(sdr_latent, **kw).images.clone()
    canon = FR.canonical(og, RANK, SEED, ADAPTERS["all"][1])
    sd = FR.to_convention(canon, "kohya", conv_names=FR.conv_targets(og))
    with pytest.raises(NotImplementedError, match="targets='transformer'"):
        pipe.load_lora_weights(sd)
    pipe.load_lora_weights(sd, targets="transformer")
    assert len(pipe.unet._lora_raw) == 12 * 16
    adapted = pipe(sdr_latent, **kw).images.clone()
    assert rms(adapted, plain) > 1e-2
    # scale 0: every update contributes exactly nothing, but the adapted blocks still take their own launches (the pre-activation
    # [tokens, 8C] is rounded to bfloat16 in front of the GEGLU, proj_out's GroupNorm computes its own statistics), so the run equals
    # the run without an adapter up to bfloat16 rounding carried through four steps, not bit for bit: gated against the adapter's effect
    off = pipe(sdr_latent, cross_attention_kwargs={"scale": 0.0}, **kw).images.clone()
    print(f"GM pipeline: adapter moves the latents by rms {rms(adapted, plain):.3e}, scale 0 leaves {rms(off, plain):.3e}")
    assert rms(off, plain) < 0.2 * rms(adapted, plain)
    pipe.unload_lora_weights()
    assert torch.equal(pipe(sdr_latent, **kw).images, plain)
