"""GPU: ControlNet conditioning on the HIP path -- the fused concat kernel bit for bit against torch's expression (with its write
footprint), the in-kernel statistics entry by entry, ``ControlNetModel`` and the UNet with residuals against the CPU references of
tests/controlnet_ref.py, and the dual pipeline with a ControlNet (graphs, guidance window, guess mode, scale rewrite)."""
import functools

import pytest
import torch

import controlnet_ref as R
import parity as P
import small_ref as S
import stats_handoff as SH

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
LAP = 2048 * 256  # csrc/controlnet.hip grid_for: 16-byte vectors per grid-stride lap
GUARD = 4096      # elements of NaN before and after a guarded output


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rms(a, b):
    return float(((a.double().cpu() - b.double().cpu()) ** 2).mean().sqrt())


# the tolerances of tests/test_models_gpu.py (relative L2 error against the float32 CPU oracle)
MODEL_TOL = {F32: 3e-5, BF16: 4e-2, F16: 6e-3}


# ---------------------------------------------------------------------------------------------------------------------------
# gmd_concat_channels_add
# ---------------------------------------------------------------------------------------------------------------------------
SCALES = [9.0, 1.0, 0.3, 0.0, 0.7, 1.0, 0.3, 0.0, 2.0, 0.3, 1.0, 0.0, 0.3]  # index 0 is never used by the cases below


def _operands(dtype, rows, Ca, Cb, r_row0, seed):
    g = torch.Generator().manual_seed(seed)
    mk = lambda n, c: torch.randn(n, c, generator=g).to(dtype)
    a, b, ra, rb = mk(rows, Ca), mk(rows, Cb), mk(rows - r_row0, Ca), mk(rows - r_row0, Cb)
    s, r = R.edge_values(dtype)  # the edge pairs in the first residual rows' leading channels, of both parts
    n = s.numel()
    for skip, res in ((a, ra), (b, rb)):
        skip[r_row0, :n], res[0, :n] = s, r
        skip[r_row0 + 1, -n:], res[1, -n:] = s, r
    return a, b, ra, rb


def _guarded(numel, dtype):
    buf = torch.full((numel + 2 * GUARD,), float("nan"), dtype=dtype, device=DEV)
    return buf, buf[GUARD:GUARD + numel]


def _launch(a, b, ra, rb, ia, ib, scales, r_row0, out, stats=None, bucket=0):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import check, lib

    p = lambda t: None if t is None else t.data_ptr()
    rows = a.shape[0]
    check(lib().gmd_concat_channels_add(p(a), a.shape[1], p(ra), ia, p(b), b.shape[1], p(rb), ib, p(scales), r_row0, p(out),
                                        ops.dtype_code(a.dtype), rows, p(stats), bucket, torch.cuda.current_stream().cuda_stream),
          "gmd_concat_channels_add")


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
@pytest.mark.parametrize("Ca,Cb", [(24, 40), (64, 128)])
@pytest.mark.parametrize("r_row0", [0, 64])
def test_concat_channels_add_is_torchs_expression_bit_for_bit(dtype, Ca, Cb, r_row0):
    rows = 128
    a, b, ra, rb = _operands(dtype, rows, Ca, Cb, r_row0, seed=Ca + r_row0)
    scales = torch.tensor(SCALES, dtype=F32)
    d = lambda t: None if t is None else t.to(DEV)
    sd = scales.to(DEV)
    for with_ra in (True, False):
        for ia, ib in ((1, 2), (2, 3), (3, 5), (12, 9)):  # 1.0 / 0.3, 0.3 / 0.0, 0.0 / 1.0, 0.3 / 0.3
            buf, out = _guarded(rows * (Ca + Cb), dtype)
            before = buf.clone()
            _launch(d(a), d(b), d(ra) if with_ra else None, d(rb), ia, ib, sd, r_row0, out)
            what = f"{dtype} {Ca}+{Cb} r_row0={r_row0} Ra={with_ra} scales[{ia}], [{ib}]"
            R.assert_concat(out.view(rows, Ca + Cb), a, b, ra if with_ra else None, rb, scales, ia, ib, r_row0, what)
            iv = {2: torch.int16, 4: torch.int32}[buf.element_size()]
            assert torch.equal(buf[:GUARD].view(iv), before[:GUARD].view(iv)), what + ": the guard band before the output changed"
            assert torch.equal(buf[-GUARD:].view(iv), before[-GUARD:].view(iv)), what + ": the guard band after the output changed"
    # no residual at all: the plain concat
    buf, out = _guarded(rows * (Ca + Cb), dtype)
    _launch(d(a), d(b), None, None, 0, 0, None, 0, out)
    S.assert_bit_equal(out.view(rows, Ca + Cb), torch.cat([a, b], -1), "no residuals")


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_concat_channels_add_second_lap(dtype):
    """More vectors than one lap of the kernel's own grid (2048 workgroups of 256 threads), residual rows starting mid-tensor."""
    from gm_diffusion import hip_ops as ops

    Ca, Cb = 24, 40
    V = 4 if dtype == F32 else 8
    rows = LAP // ((Ca + Cb) // V) + 333
    assert rows * ((Ca + Cb) // V) > LAP
    r_row0 = rows // 2 + 1
    a, b, ra, rb = _operands(dtype, rows, Ca, Cb, r_row0, seed=11)
    scales = torch.tensor(SCALES, dtype=F32)
    out = ops.concat_channels_add(a.to(DEV), b.to(DEV), ra=ra.to(DEV), rb=rb.to(DEV), ia=12, ib=4, scales=scales.to(DEV), r_row0=r_row0)
    assert getattr(out, "_colstats", None) is None
    R.assert_concat(out, a, b, ra, rb, scales, 12, 4, r_row0, f"second lap {dtype}")


def test_concat_channels_add_refuses_bad_arguments():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import HipExtensionError

    a, b = torch.zeros(64, 24, dtype=BF16, device=DEV), torch.zeros(64, 40, dtype=BF16, device=DEV)
    sc = torch.ones(13, device=DEV)
    for kw in (dict(rb=torch.zeros(64, 40, dtype=BF16, device=DEV), ib=13, scales=sc), dict(rb=torch.zeros(32, 40, dtype=BF16, device=DEV), scales=sc),
               dict(rb=torch.zeros(64, 40, dtype=BF16, device=DEV)), dict(r_row0=65), dict(rb=torch.zeros(64, 40, dtype=F16, device=DEV), scales=sc)):
        with pytest.raises(HipExtensionError):
            ops.concat_channels_add(a, b, **kw)
    with pytest.raises(HipExtensionError):  # channel counts that are no multiple of a 16-byte vector: refused before a launch
        _launch(a[:, :20].contiguous(), b, None, None, 0, 0, None, 0, torch.empty(64 * 60, dtype=BF16, device=DEV))
    st = torch.empty(64, dtype=F32, device=DEV)
    with pytest.raises(HipExtensionError):  # Cb = 20 with statistics: fine in float32, not a whole number of 16-bit vectors
        _launch(b, a[:, :20].contiguous(), None, None, 0, 0, None, 0, torch.empty(64 * 60, dtype=BF16, device=DEV), stats=st, bucket=10)
    with pytest.raises(HipExtensionError):  # a bucket that does not divide Cb
        _launch(a, b, None, None, 0, 0, None, 0, torch.empty(64 * 64, dtype=BF16, device=DEV), stats=st, bucket=16)


# ---------------------------------------------------------------------------------------------------------------------------
# statistics of the stored B part
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,rows,Cb", [(F32, 128, 20), (F32, 256, 40), (BF16, 256, 40), (F16, 256, 40)])
def test_statistics_every_entry_written_and_within_its_bound(dtype, rows, Cb):
    """Two operand sets alternating on ONE statistics buffer, NaN-filled before every launch: a stale or unwritten entry shows.
    (Cb = 20 is two buckets and five float32 vectors; it is no multiple of a 16-bit vector of 8, so the 16-bit types cannot take it:
    test_concat_channels_add_refuses_bad_arguments has that refusal.)"""
    Ca = 40
    scales = torch.tensor(SCALES, dtype=F32)
    sets = [_operands(dtype, rows, Ca, Cb, 0, seed) for seed in (21, 22)]
    sets[1] = tuple(t * 3 for t in sets[1])  # the two sets' sums differ by far more than any bound
    extent = rows // 64 * (Cb // 10) * 2
    st = torch.empty(extent + 64, dtype=F32, device=DEV)
    out = torch.empty(rows, Ca + Cb, dtype=dtype, device=DEV)
    for k in (0, 1, 0, 1):
        a, b, ra, rb = (t.to(DEV) for t in sets[k])
        SH.nan_fill(st)
        _launch(a, b, None, rb, 0, 4, scales.to(DEV), 0, out, stats=st, bucket=10)
        what = f"{dtype} rows={rows} Cb={Cb} set {k}"
        R.assert_concat(out, sets[k][0], sets[k][1], None, sets[k][3], scales, 0, 4, 0, what)
        assert SH.unwritten(st, extent).numel() == 0, what + ": unwritten entries"
        R.assert_stats(st[:extent].view(rows // 64, Cb // 10, 2), out[:, Ca:].float().cpu(), 10, what)


@pytest.fixture
def concat_stats():
    """The in-kernel statistics of the fused concat are off by default (they do not pay: profiles/controlnet.txt): on for the test."""
    from gm_diffusion import hip_ops as ops

    prev, ops.USE_CONCAT_STATS = ops.USE_CONCAT_STATS, True
    yield
    ops.USE_CONCAT_STATS = prev


def test_in_kernel_statistics_are_off_by_default_and_then_nothing_is_attached():
    from gm_diffusion import hip_ops as ops

    assert ops.USE_CONCAT_STATS is False
    a, b = torch.zeros(2, 64, 40, dtype=BF16, device=DEV), torch.zeros(2, 64, 40, dtype=BF16, device=DEV)
    a._colstats = (torch.zeros(2, 4, 2, device=DEV), 40)
    b._colstats = (torch.zeros(2, 4, 2, device=DEV), 40)
    x = ops.concat_channels_add(a, b, rb=torch.ones(2, 64, 40, dtype=BF16, device=DEV), ib=1, scales=torch.ones(13, device=DEV), hw=64)
    assert getattr(x, "_colstats", None) is None  # never the skip producer's statistics


@pytest.mark.parametrize("dtype", [BF16, F32])
def test_groupnorm_takes_the_fresh_statistics_and_agrees_with_the_general_path(dtype, concat_stats):
    from gm_diffusion import hip_ops as ops

    B, HW, Ca, Cb, G = 2, 64, 40, 40, 4
    a, b, ra, rb = _operands(dtype, B * HW, Ca, Cb, 0, seed=31)
    scales = torch.tensor(SCALES, dtype=F32).to(DEV)
    g = torch.Generator().manual_seed(32)
    gamma, beta = (torch.rand(Ca + Cb, generator=g) + 0.5).to(DEV), torch.randn(Ca + Cb, generator=g).to(DEV)
    da = a.to(DEV).view(B, HW, Ca)
    da._colstats = (SH.bucket_sums(a, 10).float().to(DEV), Ca)  # what A's producer would have left: A is not modified here
    x = ops.concat_channels_add(da, b.to(DEV).view(B, HW, Cb), rb=rb.to(DEV), ib=4, scales=scales, hw=HW)
    st = x._colstats
    assert isinstance(st, list) and st[0] is da._colstats and st[1][1] == Cb and st[1][0].shape == (B * HW // 64, Cb // 10, 2)
    R.assert_stats(st[1][0], x.view(B * HW, -1)[:, Ca:].float().cpu(), 10, "fresh statistics")
    before = ops.colstats_uses
    y_stats = ops.groupnorm(x, B, G, gamma, beta, 1e-5, silu=True)
    assert ops.colstats_uses == before + 1
    plain = x.clone()
    y_general = ops.groupnorm(plain, B, G, gamma, beta, 1e-5, silu=True)
    assert ops.colstats_uses == before + 1
    # one float64 reference, each path inside ITS bound: the statistics path sums along the producers' chain (44 additions), the
    # general path along some tree over the group's HW * C / G values (at most that many additions)
    for y, height, what in ((y_stats, SH.producer_height(10), "statistics path"), (y_general, HW * (Ca + Cb) // G, "general path")):
        ref, bound = P.groupnorm_ref_bound(x.cpu(), G, gamma.cpu(), beta.cpu(), 1e-5, dtype, height, True)
        P.assert_elementwise(y.cpu(), ref, bound, what)
    # a modified part never passes statistics on: with Ra nothing is attached, and nothing when the fresh ones cannot be made
    db = b.to(DEV).view(B, HW, Cb)
    db._colstats = (SH.bucket_sums(b, 10).float().to(DEV), Cb)
    with_ra = ops.concat_channels_add(da, db, ra=ra.to(DEV), rb=rb.to(DEV), ia=12, ib=4, scales=scales, hw=HW)
    assert getattr(with_ra, "_colstats", None) is None
    only_ra = ops.concat_channels_add(da, db, ra=ra.to(DEV), ia=12, scales=scales, hw=HW)
    assert getattr(only_ra, "_colstats", None) is None
    no_hw = ops.concat_channels_add(da, db, rb=rb.to(DEV), ib=4, scales=scales)
    assert getattr(no_hw, "_colstats", None) is None  # never the skip producer's stale statistics
    untouched = ops.concat_channels_add(da, db)
    assert untouched._colstats[0] is da._colstats and untouched._colstats[1] is db._colstats  # no residual: as concat_channels


def test_silu_in_place_matches_the_groupnorm_kernels_formula():
    from gm_diffusion import hip_ops as ops

    for dtype in (F32, BF16, F16):
        x = (torch.randn(3, 40, 16, generator=torch.Generator().manual_seed(1)) * 4).to(dtype)
        y = ops.silu_(x.to(DEV).clone())
        ref = torch.nn.functional.silu(x.double())
        # parity.py's bound of store(silu(v)) at an exact argument: silu_f's evaluation error and the one rounding of the store
        bound = P._finish(x.double(), torch.zeros_like(ref), dtype, "silu")
        P.assert_elementwise(y.cpu(), ref, bound, f"silu {dtype}")


# ---------------------------------------------------------------------------------------------------------------------------
# models
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refs():
    from oracle import fixtures

    torch.manual_seed(5)
    cn = R.ControlNetRef(**R.tiny_controlnet_config()).eval().requires_grad_(False)
    return cn, fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8)


def _hip_cn(ref, dtype):
    from gm_diffusion.components import ControlNetModel

    m = ControlNetModel(**R.tiny_controlnet_config())
    m.load_state_dict(ref.state_dict())
    return m.to(DEV, dtype)


def _hip_unet(ou, dtype):
    from gm_diffusion.components import UNet2DConditionModel

    m = UNet2DConditionModel(**vars(ou.config))
    m.load_state_dict(ou.state_dict())
    return m.to(DEV, dtype)


@functools.lru_cache(maxsize=None)
def _model_case(h, w):
    """Inputs and the CPU references of one latent size, computed once."""
    cn, ou, _ = _refs()
    g = torch.Generator().manual_seed(40 + h)
    x, ctx, img = torch.randn(2, 4, h, w, generator=g), torch.randn(2, 77, 64, generator=g), torch.rand(2, 3, 8 * h, 8 * w, generator=g)
    with torch.no_grad():
        down, mid = cn(x, torch.tensor(501), ctx, img, conditioning_scale=0.8)
        gdown, gmid = cn(x, torch.tensor(501), ctx, img, conditioning_scale=0.8, guess_mode=True)
        eps = R.unet_forward_with_residuals(ou, x, torch.tensor(501), ctx, down, mid)
        plain = R.unet_forward_with_residuals(ou, x, torch.tensor(501), ctx)
    return x, ctx, img, down, mid, gdown, gmid, eps, plain


@pytest.mark.parametrize("dtype,mode", [(F32, "split"), (F32, "exact"), (BF16, "split"), (F16, "split")])
@pytest.mark.parametrize("h,w", [(8, 8), (6, 10)])
def test_controlnet_and_unet_with_residuals_against_the_references(dtype, mode, h, w):
    from gm_diffusion import hip_ops as ops

    prev = ops.set_f32_mode(mode)
    try:
        cn_ref, ou, _ = _refs()
        x, ctx, img, down, mid, gdown, gmid, eps, plain = _model_case(h, w)
        tol = MODEL_TOL[dtype]
        cn, hu = _hip_cn(cn_ref, dtype), _hip_unet(ou, dtype)
        dx, dctx, dimg = x.to(DEV), ctx.to(DEV), img.to(DEV)
        got = cn(dx, 501, dctx, dimg, conditioning_scale=0.8)
        assert len(got.down_block_res_samples) == 12 and got.mid_block_res_sample.dtype == dtype
        for k, (a, b) in enumerate(zip(list(got.down_block_res_samples) + [got.mid_block_res_sample], down + [mid])):
            assert a.shape == b.shape and rel_err(a.float(), b) < tol, (k, rel_err(a.float(), b))
        gg = cn(dx, 501, dctx, dimg, conditioning_scale=0.8, guess_mode=True, return_dict=False)
        for k, (a, b) in enumerate(zip(list(gg[0]) + [gg[1]], gdown + [gmid])):
            assert rel_err(a.float(), b) < tol, ("guess", k, rel_err(a.float(), b))
        # the UNet with the REFERENCE residuals against the restated forward; then with its own ControlNet's residuals (e2: the
        # value the packed and the captured paths below must reproduce bit for bit)
        e1 = hu(dx, 501, encoder_hidden_states=dctx, down_block_additional_residuals=[t.to(DEV) for t in down],
                mid_block_additional_residual=mid.to(DEV), return_dict=False)[0]
        assert e1.shape == eps.shape and rel_err(e1, eps) < tol, rel_err(e1, eps)
        e2 = hu(dx, 501, encoder_hidden_states=dctx, down_block_additional_residuals=got.down_block_res_samples,
                mid_block_additional_residual=got.mid_block_res_sample, return_dict=False)[0]
        assert rel_err(plain, eps) > 100 * MODEL_TOL[F32]  # (the references themselves: the residuals matter)
        # the packed path (unscaled buffers, the scale applied by the UNet's concat kernel) gives the public path's bits
        c = cn.prepare_context(dctx)
        cn.set_timestep(501)
        cn.set_condition(dimg, 2)
        pdown, pmid = cn.forward_packed(cn.pack_input(dx), 2, h, w, c)
        sc = cn.set_scales(0.8, False)
        hu.set_timestep(501)
        e3 = hu.forward_packed(hu.pack_input(dx), 2, h, w, hu.prepare_context(dctx), control=(pdown, pmid, sc, 0))
        assert torch.equal(e3, e2)
        # captured: ControlNet graph, then the UNet's control graph, reading the static buffers and the device scales
        gc = cn.graphed_forward(2, h, w, c)
        gu = hu.graphed_forward(2, h, w, hu.prepare_context(dctx), control=(gc.down, gc.mid, sc, 0))
        cn.pack_input(dx, out=gc.x)
        hu.pack_input(dx, out=gu.x)
        gc.replay()
        assert torch.equal(gu.replay(), e2)
        n_graphs = len(hu._graphs)
        cn.set_scales(0.0, False)  # rewritten outside the graph: no recapture, the plain forward's values
        assert hu.graphed_forward(2, h, w, hu.prepare_context(dctx), control=(gc.down, gc.mid, sc, 0)) is gu and len(hu._graphs) == n_graphs
        zero = gu.replay().clone()
        assert torch.equal(zero, hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0])
    finally:
        ops.set_f32_mode(prev)


def test_guess_mode_skips_the_unconditional_half():
    """``skip_samples``: residuals of the conditional half only, the first half of the batch a plain copy."""
    cn_ref, ou, _ = _refs()
    x, ctx, img = _model_case(8, 8)[:3]
    cn, hu = _hip_cn(cn_ref, F32), _hip_unet(ou, F32)
    dx, dctx, dimg = x.to(DEV), ctx.to(DEV), img.to(DEV)
    c = cn.prepare_context(dctx[1:])
    cn.set_timestep(301)
    cn.set_condition(dimg[1:], 1)
    pdown, pmid = cn.forward_packed(cn.pack_input(dx[1:]), 1, 8, 8, c)
    sc = cn.set_scales(1.0, True)
    hu.set_timestep(301)
    uc = hu.prepare_context(dctx)
    both = hu.forward_packed(hu.pack_input(dx), 2, 8, 8, uc, control=(pdown, pmid, sc, 1))
    plain = hu.forward_packed(hu.pack_input(dx), 2, 8, 8, uc)
    assert torch.equal(both[0], plain[0]) and not torch.equal(both[1], plain[1])
    with torch.no_grad():
        d, m = cn_ref(x[1:], torch.tensor(301), ctx[1:], img[1:], guess_mode=True)
        d = [torch.cat([torch.zeros_like(t), t]) for t in d]
        ref = R.unet_forward_with_residuals(ou, x, torch.tensor(301), ctx, d, torch.cat([torch.zeros_like(m), m]))
    assert rel_err(both, ref) < MODEL_TOL[F32]


def test_unet_takes_the_fresh_statistics_where_a_level_has_them():
    """SD-1.5's first-level width (320, 32 groups) at 64x64 latents, UNet batch 4: the level whose GroupNorms read producer statistics.
    With a ControlNet the up blocks' first GroupNorm must be served from the concat kernel's fresh statistics (the count of GroupNorms
    on the statistics path drops when the in-kernel statistics are switched off) and agree with the general route to the tolerance
    tests/test_models_gpu.py holds the producer statistics to against the statistics launch (bfloat16: 1.5e-2)."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components import ControlNetModel, UNet2DConditionModel

    cfg = dict(block_out_channels=(320, 320, 320, 320), cross_attention_dim=64, attention_head_dim=8, norm_num_groups=32)
    hu = UNet2DConditionModel(**cfg).init_random(3, device=DEV).to(DEV, BF16)
    cn = ControlNetModel(**cfg, conditioning_embedding_out_channels=(8, 8, 16, 16)).init_random(4, device=DEV).to(DEV, BF16)
    g = torch.Generator().manual_seed(6)
    B, h = 4, 64
    x, ctx = torch.randn(B, 4, h, h, generator=g).to(DEV), torch.randn(B, 77, 64, generator=g).to(DEV)
    img = torch.rand(B, 3, 8 * h, 8 * h, generator=g).to(DEV)
    c = cn.prepare_context(ctx)
    cn.set_timestep(401)
    cn.set_condition(img, B)
    down, mid = cn.forward_packed(cn.pack_input(x), B, h, h, c)
    sc = cn.set_scales(1.0, False)
    hu.set_timestep(401)
    uc = hu.prepare_context(ctx)
    px = hu.pack_input(x)
    out, used = {}, {}
    prev = ops.USE_CONCAT_STATS
    for use in (True, False):
        ops.USE_CONCAT_STATS = use
        try:
            before = ops.colstats_uses
            out[use] = hu.forward_packed(px, B, h, h, uc, control=(down, mid, sc, 0))
            used[use] = ops.colstats_uses - before
        finally:
            ops.USE_CONCAT_STATS = prev
    before = ops.colstats_uses
    plain = hu.forward_packed(px, B, h, h, uc)
    used_plain = ops.colstats_uses - before
    print(f"GroupNorms on the statistics path: plain {used_plain}, control {used[True]}, control without in-kernel statistics {used[False]}")
    assert used[True] > used[False] and used[True] <= used_plain
    assert rel_err(out[True], out[False]) < 1.5e-2, rel_err(out[True], out[False])
    assert rel_err(out[True], plain) > 10 * 1.5e-2  # the residuals move the result by far more than that tolerance


# ---------------------------------------------------------------------------------------------------------------------------
# pipeline
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = 4


def _pndm():
    from gm_diffusion.components import PNDMScheduler

    return PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True, steps_offset=1,
                         set_alpha_to_one=False)


def _pipe(dtype, controlnet="ref"):
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    cn_ref, ou, og = _refs()
    cn = _hip_cn(cn_ref, dtype) if controlnet == "ref" else controlnet
    pipe = StableDiffusionDualUNetPipeline(vae=None, text_encoder=None, tokenizer=None, unet=_hip_unet(ou, dtype), gm_unet=_hip_unet(og, dtype),
                                           scheduler=_pndm(), safety_checker=None, feature_extractor=None, requires_safety_checker=False,
                                           controlnet=cn)
    pipe.set_progress_bar_config(disable=True)
    return pipe


@functools.lru_cache(maxsize=None)
def _pipe_inputs():
    from oracle import fixtures

    pos, neg, lat = fixtures.make_inputs(1, 8, 8, cross_dim=64)
    img = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(8))
    return pos, neg, lat, img


def _kw(**extra):
    pos, neg, lat, img = _pipe_inputs()
    return dict(prompt_embeds=pos.to(DEV), negative_prompt_embeds=neg.to(DEV), latents=lat.to(DEV), height=64, width=64,
                num_inference_steps=STEPS, guidance_scale=7.5, output_type="latent", control_image=img.to(DEV), **extra)


@functools.lru_cache(maxsize=None)
def _ref_loop(controlnet=True, **kw):
    from oracle import schedulers as osched

    cn_ref, ou, og = _refs()
    pos, neg, lat, img = _pipe_inputs()
    return R.dual_loop_controlnet(ou, og, cn_ref if controlnet else None, osched.PNDMScheduler(), pos, neg, lat, img,
                                  num_inference_steps=STEPS, guidance_scale=7.5, **kw)


def test_pipeline_graphs_and_streams_equal_eager_bit_for_bit():
    pipe = _pipe(BF16)
    pipe.co_run_plans = True  # one plan family for every mode
    pipe.use_hip_graphs, pipe.overlap_streams = False, False
    a = pipe(**_kw(controlnet_conditioning_scale=0.8))
    pipe.use_hip_graphs, pipe.overlap_streams = True, True
    b = pipe(**_kw(controlnet_conditioning_scale=0.8))
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    # guess mode likewise (the ControlNet at half the UNet's batch, the unconditional samples skipped by the concat kernel)
    pipe.use_hip_graphs, pipe.overlap_streams = False, False
    c = pipe(**_kw(guess_mode=True))
    pipe.use_hip_graphs, pipe.overlap_streams = True, True
    d = pipe(**_kw(guess_mode=True))
    torch.cuda.synchronize()
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1]) and not torch.equal(c[0], a[0])


@pytest.mark.parametrize("guess_mode", [False, True])
def test_pipeline_f32_against_the_restated_cpu_loop(guess_mode):
    pipe = _pipe(F32)
    sdr, gm = pipe(**_kw(guess_mode=guess_mode))
    ref_sdr, ref_gm = _ref_loop(guess_mode=guess_mode)
    e_sdr, e_gm = rms(sdr, ref_sdr), rms(gm, ref_gm)
    print(f"controlnet pipeline (guess_mode={guess_mode}) latent RMS vs the CPU loop: sdr={e_sdr:.3e} gm={e_gm:.3e}")
    assert e_sdr <= 1e-3 and e_gm <= 1e-3
    plain_sdr, _ = _ref_loop(controlnet=False)
    assert rms(ref_sdr, plain_sdr) > 1e-2  # the conditioning moves the result by far more than the gate
    other_sdr, _ = _ref_loop(guess_mode=not guess_mode)
    assert rms(ref_sdr, other_sdr) > 1e-2  # and the two modes differ
    # the generic (non-fused) loop through the public __call__s
    pipe._use_fused = lambda *args: False
    sdr2, gm2 = pipe(**_kw(guess_mode=guess_mode))
    assert rms(sdr2, ref_sdr) <= 1e-3 and rms(gm2, ref_gm) <= 1e-3


def test_pipeline_from_unet_zero_scale_and_window():
    from gm_diffusion.components import ControlNetModel

    plain_pipe = _pipe(F32, controlnet=None)
    probe = {}

    def record(name):
        probe[name] = []
        return lambda i, s, g: probe[name].append((s.clone(), g.clone()))

    plain_pipe._step_probe = record("plain")
    plain = plain_pipe(**_kw())  # (the five keywords are ignored without a controlnet)
    n_steps = len(probe["plain"])
    # from_unet: zero residuals -> the plain run, by value
    zero_cn = ControlNetModel.from_unet(plain_pipe.unet, conditioning_embedding_out_channels=(8, 8, 16, 16))
    z = _pipe(F32, controlnet=zero_cn)(**_kw())
    assert torch.equal(z[0], plain[0]) and torch.equal(z[1], plain[1])
    # a live ControlNet inside a window starting at 0.5: identical to the plain run up to the window, different after it
    pipe = _pipe(F32)
    pipe._step_probe = record("window")
    w = pipe(**_kw(control_guidance_start=0.5))
    keep = R.keep_window(n_steps, 0.5, 1.0)
    assert not keep[0] and keep[-1] and len(probe["window"]) == n_steps
    first = keep.index(True)
    for i in range(n_steps):
        same = torch.equal(probe["window"][i][0], probe["plain"][i][0])
        assert same == (i < first), (i, first)
    assert torch.equal(probe["window"][first - 1][1], probe["plain"][first - 1][1]) and not torch.equal(w[1], plain[1])
    # scale 0.0 on the same pipeline: the plain run by value, from the graphs it already has
    pipe._step_probe = None
    live = pipe(**_kw())
    assert not torch.equal(live[0], plain[0])
    counts = (len(pipe.unet._graphs), len(pipe.controlnet._graphs), len(pipe.gm_unet._graphs))
    off = pipe(**_kw(controlnet_conditioning_scale=0.0))
    assert torch.equal(off[0], plain[0]) and torch.equal(off[1], plain[1])
    assert (len(pipe.unet._graphs), len(pipe.controlnet._graphs), len(pipe.gm_unet._graphs)) == counts
    again = pipe(**_kw())
    assert torch.equal(again[0], live[0]) and torch.equal(again[1], live[1])


def test_no_controlnet_launches_what_it_launched_before():
    """controlnet=None: per kind, a step launches exactly the two UNets' plain forwards (twelve ``gmd_concat_channels`` per forward,
    one per up-block resnet, and not one launch of the fused concat) -- with or without the five keywords."""
    from gm_diffusion import hip_ops as ops, profiling

    pipe = _pipe(BF16, controlnet=None)
    pos, neg, lat, img = _pipe_inputs()

    def histogram(fn):
        t = profiling.KernelTimer()
        profiling.set_timer(t)
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            profiling.set_timer(None)
        h = {}
        for rec in t.records:
            h[rec[0]] = h.get(rec[0], 0) + 1
        return h

    calls = {"add": 0}
    real = ops.concat_channels_add
    ops.concat_channels_add = lambda *a, **k: (calls.__setitem__("add", calls["add"] + 1), real(*a, **k))[1]
    try:
        with_kw = histogram(lambda: pipe(**_kw(guess_mode=True, controlnet_conditioning_scale=0.5)))
        kw = _kw()
        kw.pop("control_image")
        without = histogram(lambda: pipe(**kw))
    finally:
        ops.concat_channels_add = real
    assert with_kw == without and calls["add"] == 0
    hu, hg = pipe.unet, pipe.gm_unet
    ctx = hu.prepare_context(torch.cat([neg, pos]).to(DEV))
    hu.set_timestep(500)
    hg.set_timestep(500)
    shared = pipe._cfg_shared(hu, True)
    x = hu.pack_input(lat.to(DEV), dup=1 if shared else 2)
    gx = hg.pack_input((lat.to(DEV), lat.to(DEV)))
    gctx = hg.prepare_context(pos.to(DEV))
    hu.update_context(ctx), hg.update_context(gctx)
    one_sdr = histogram(lambda: hu.forward_packed(x, 2, 8, 8, ctx, cfg_shared=shared))
    one_gm = histogram(lambda: hg.forward_packed(gx, 1, 8, 8, gctx))
    assert one_sdr["concat"] == 12 and one_gm["concat"] == 12
    n_iter = len(pipe.scheduler.timesteps)
    for kind in ("concat", "conv3x3", "groupnorm", "layernorm"):
        assert without[kind] == n_iter * (one_sdr[kind] + one_gm[kind]), kind
