"""GPU: IP-Adapter image prompting.  The fused decoupled cross-attention kernel (gmd_attention_ip) per element against the float64
reference and the bound of tests/ip_adapter_ref.py; branch independence; its write footprint; the device-resident scale; the composed
routes; the image-prompted UNet against the oracle's; the dual-UNet pipeline against the restated CPU loop."""
import functools

import pytest
import torch

import ip_adapter_ref as R
import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
MODEL_TOL = {F32: 2e-5, BF16: 3e-2, F16: 4e-3}  # tests/test_models_gpu.py: the tiny UNet against the oracle, per dtype
GUARD = 4096  # elements of NaN before and after a guarded output


def rel_err(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / (b.norm() + 1e-30))


def rms(a, b):
    return float(((a.double().cpu() - b.double().cpu()) ** 2).mean().sqrt())


def _pad8(n):
    return (n + 7) // 8 * 8


def _rows(t, ld, col, fill=float("nan")):
    """[B, H, N, D] -> a device buffer [B, N, ld] holding the heads at columns [col, col + H*D), everything else ``fill``."""
    B, H, N, D = t.shape
    buf = torch.full((B, N, ld), fill, dtype=t.dtype, device=DEV)
    buf[:, :, col:col + H * D] = t.permute(0, 2, 1, 3).reshape(B, N, H * D).to(DEV)
    return buf


def _vt(t, ld):
    """[B, H, N, D] -> V^T [B, H*D, ld] with zero pad columns."""
    B, H, N, D = t.shape
    buf = torch.zeros((B, H * D, ld), dtype=t.dtype, device=DEV)
    buf[:, :, :N] = t.permute(0, 1, 3, 2).reshape(B, H * D, N).to(DEV)
    return buf


def _launch(q, k, v, kip, vip, scale, scales, idx, q_col=0, k_col=0, pad=0, out=None, ldo=None, vt_extra=0):
    """gmd_attention_ip through the C ABI on [B, H, N, D] operands laid out with leading dimensions ``pad`` wider than H*D and Q / K
    at a column offset; ``out``: a [B, Nq, ldo] view to store into (default: a fresh tight tensor).  Returns O as [B, H, Nq, D]."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import check, lib

    B, H, Nq, D = q.shape
    Nk, Nip = k.shape[2], kip.shape[2]
    hd = H * D
    qb, kb = _rows(q, q_col + hd + pad, q_col), _rows(k, k_col + hd + pad, k_col)
    kipb = _rows(kip, hd + pad, 0)
    vtb, vtipb = _vt(v, _pad8(Nk) + vt_extra), _vt(vip, _pad8(Nip) + vt_extra)
    ldo = ldo or hd
    if out is None:
        out = torch.empty((B, Nq, ldo), dtype=q.dtype, device=DEV)
    es = q.element_size()
    check(lib().gmd_attention_ip(qb.data_ptr() + q_col * es, kb.data_ptr() + k_col * es, vtb.data_ptr(), kipb.data_ptr(), vtipb.data_ptr(),
                                 out.data_ptr(), ops.dtype_code(q.dtype), B, H, D, Nq, Nk, Nip, qb.shape[2], kb.shape[2], vtb.shape[2],
                                 kipb.shape[2], vtipb.shape[2], ldo, Nq * qb.shape[2], Nk * kb.shape[2], hd * vtb.shape[2],
                                 Nip * kipb.shape[2], hd * vtipb.shape[2], Nq * ldo, float(scale), scales.data_ptr(), int(idx),
                                 torch.cuda.current_stream().cuda_stream), "gmd_attention_ip")
    torch.cuda.synchronize()
    return out[:, :, :hd].reshape(B, Nq, H, D).permute(0, 2, 1, 3)


def _scales(value, idx, n=16):
    """A 16-entry device array with ``value`` at ``idx`` and a value that would be noticed (1e4) everywhere else."""
    s = torch.full((n,), 1.0e4, dtype=torch.float32)
    s[idx] = value
    return s.to(DEV)


# ---------------------------------------------------------------------------------------------------------------------------
# kernel, per element
# ---------------------------------------------------------------------------------------------------------------------------
NQ, NK, NIP = (1, 64, 161), (1, 64, 77, 130), (1, 4, 8, 20, 64)
# pairwise covering: every (Nk, Nip) pair once, Nq = (i + j) mod 3 walks all three values along every row and column of that table
SHAPES = [(NQ[(i + j) % 3], NK[i], NIP[j]) for i in range(4) for j in range(5)]
IP_SCALES = (0.0, 1.0, 0.6, -0.5)


def test_shape_table_is_pairwise_covering():
    assert {(a, b) for a, b, _ in SHAPES} == {(a, b) for a in NQ for b in NK}
    assert {(a, c) for a, _, c in SHAPES} == {(a, c) for a in NQ for c in NIP}
    assert {(b, c) for _, b, c in SHAPES} == {(b, c) for b in NK for c in NIP}


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", [32, 40, 64, 80, 160])
def test_kernel_per_element_zero_violations(D, dtype):
    """B = 2, H = 2; the 20 pairwise-covering (Nq, Nk, Nip) for every head dim and both types; ldq / ldk / ldkip 24 wider than H*D, Q
    and K at column offsets 16 and 8 of their buffers (NaN everywhere around them), ldo = H*D + 8; the four scales, read at index 0
    and at the last index of a 16-entry array whose other entries are 1e4."""
    scale = D ** -0.5
    worst = 0.0
    for c, (Nq, Nk, Nip) in enumerate(SHAPES):
        ip_scale, idx = IP_SCALES[c % 4], (0, 15)[(c // 4 + c) % 2]
        q, k, v, kip, vip = R.make_qkv(2, 2, Nq, Nk, Nip, D, dtype, seed=1000 * D + c)
        got = _launch(q, k, v, kip, vip, scale, _scales(ip_scale, idx), idx, q_col=16, k_col=8, pad=24, ldo=2 * D + 8)
        ref, bound = R.decoupled_bound(q.to(DEV), k.to(DEV), v.to(DEV), kip.to(DEV), vip.to(DEV), scale, ip_scale, dtype)
        worst = max(worst, P.assert_elementwise(got, ref, bound, f"attention_ip D={D} {dtype} Nq={Nq} Nk={Nk} Nip={Nip} s={ip_scale}[{idx}]",
                                                tile=(32, 8)))
    print(f"attention_ip D={D} {dtype}: max |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", [40, 64, 160])
@pytest.mark.parametrize("image_dominates", [True, False])
def test_branch_independence(D, dtype, image_dominates):
    """Every score of one branch ~40 above every score of the other: each branch must still be its own softmax.  A shared row sum
    (or, in float16, a shared stabiliser) returns ~0 for the weak branch and misses the bound by orders of magnitude."""
    scale = D ** -0.5
    q, k, v, kip, vip = R.independence_inputs(2, 2, 161, 77, 4, D, dtype, scale, image_dominates, seed=D)
    got = _launch(q, k, v, kip, vip, scale, _scales(0.6, 3), 3)
    ref, bound = R.decoupled_bound(q.to(DEV), k.to(DEV), v.to(DEV), kip.to(DEV), vip.to(DEV), scale, 0.6, dtype)
    P.assert_elementwise(got, ref, bound, f"independence D={D} {dtype} image_dominates={image_dominates}", tile=(32, 8))
    # the check has teeth: the same inputs through one softmax over all keys break it almost everywhere
    fault = R.emulate(q, k, v, kip, vip, scale, 0.6, dtype, "shared_sum").to(DEV)
    assert int(P.violations(fault, ref, bound)[0].sum()) > ref.numel() // 2


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D,Nq", [(40, 161), (160, 130), (32, 1)])
def test_write_footprint(D, Nq, dtype):
    """O inside a NaN-filled buffer with guard bands, ldo = H*D + 24: guards and pad columns keep their bits, every element of the
    window is written, and the window equals an unguarded launch bit for bit."""
    B, H, Nk, Nip = 2, 2, 77, 4
    hd, ldo = H * D, H * D + 24
    scale = D ** -0.5
    q, k, v, kip, vip = R.make_qkv(B, H, Nq, Nk, Nip, D, dtype, seed=D + Nq)
    sc = _scales(0.6, 0)
    plain = _launch(q, k, v, kip, vip, scale, sc, 0)
    buf = torch.full((2 * GUARD + B * Nq * ldo,), float("nan"), dtype=dtype, device=DEV)
    before = buf.clone()
    out = buf[GUARD:GUARD + B * Nq * ldo].view(B, Nq, ldo)
    got = _launch(q, k, v, kip, vip, scale, sc, 0, out=out, ldo=ldo)
    bits = lambda t: t.contiguous().view(torch.int16)
    assert torch.equal(bits(buf[:GUARD]), bits(before[:GUARD])) and torch.equal(bits(buf[-GUARD:]), bits(before[-GUARD:])), "guard band changed"
    assert torch.equal(bits(out[:, :, hd:]), bits(before[GUARD:GUARD + B * Nq * ldo].view(B, Nq, ldo)[:, :, hd:])), "pad columns changed"
    assert not bool(torch.isnan(out[:, :, :hd]).any()), "an element of O was never written"
    assert torch.equal(bits(got), bits(plain))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_ip_scale_zero_is_the_text_attention_and_one_graph_serves_every_scale(dtype):
    from gm_diffusion import hip_ops as ops

    B, H, Nq, Nk, Nip, D = 2, 2, 161, 77, 4, 40
    scale = D ** -0.5
    q, k, v, kip, vip = R.make_qkv(B, H, Nq, Nk, Nip, D, dtype, seed=9)
    vip = vip * 1.0e4  # a dead branch with large values: 0 * finite, no NaN
    qb, kb, kipb = _rows(q, H * D, 0), _rows(k, H * D, 0), _rows(kip, H * D, 0)
    vtb, vtipb = _vt(v, _pad8(Nk)), _vt(vip, _pad8(Nip))
    sc = torch.zeros(16, dtype=torch.float32, device=DEV)
    o0 = ops.attention_ip(qb, kb, vtb, kipb, vtipb, H, Nk, Nip, scale, sc, 5, fused=True)
    text = ops.attention(qb, kb, vtb, H, Nk, scale)
    torch.cuda.synchronize()
    assert not bool(torch.isnan(o0).any())
    ref, b_fused = R.decoupled_bound(q.to(DEV), k.to(DEV), v.to(DEV), kip.to(DEV), vip.to(DEV), scale, 0.0, dtype)
    _, b_text = P.attention_bound(q.to(DEV), k.to(DEV), v.to(DEV), scale, dtype)
    as_heads = lambda o: o.view(B, Nq, H, D).permute(0, 2, 1, 3)
    P.assert_elementwise(as_heads(o0), ref, b_fused, f"ip_scale 0 {dtype} vs the reference")
    P.assert_elementwise(as_heads(o0), as_heads(text).double(), b_fused + b_text, f"ip_scale 0 {dtype} vs ops.attention")
    # one captured launch, the scale rewritten in device memory between replays
    out = torch.empty_like(o0)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.attention_ip(qb, kb, vtb, kipb, vtipb, H, Nk, Nip, scale, sc, 5, fused=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out.copy_(ops.attention_ip(qb, kb, vtb, kipb, vtipb, H, Nk, Nip, scale, sc, 5, fused=True))
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, o0)
    sc[5] = 0.6
    g.replay()
    torch.cuda.synchronize()
    assert not torch.equal(out, o0)
    ref6, b6 = R.decoupled_bound(q.to(DEV), k.to(DEV), v.to(DEV), kip.to(DEV), vip.to(DEV), scale, 0.6, dtype)
    P.assert_elementwise(as_heads(out), ref6, b6, f"replay after the scale changed {dtype}")


def test_argument_checks_and_empty_launches():
    from gm_diffusion._native import lib

    q, k, v, kip, vip = R.make_qkv(1, 2, 8, 8, 4, 40, BF16)
    sc = _scales(1.0, 0)
    with pytest.raises(Exception, match="Nip"):
        _launch(q, k, v, R.make_qkv(1, 2, 8, 8, 65, 40, BF16)[3], R.make_qkv(1, 2, 8, 8, 65, 40, BF16)[4], 1.0, sc, 0)
    n = lib().gmd_attention_ip
    a = torch.zeros(4096, dtype=BF16, device=DEV).data_ptr()
    args = lambda **o: [o.get("Q", a), a, a, a, a, a, o.get("dtype", 1), o.get("B", 1), 2, o.get("D", 40), o.get("Nq", 8), 8, o.get("Nip", 4),
                        o.get("ldq", 80), 80, 8, 80, o.get("ldvtip", 8), 80, 640, 640, 640, 320, 640, 640, 1.0, o.get("sc", sc.data_ptr()),
                        o.get("idx", 0), None]
    assert n(*args()) == 0
    assert n(*args(B=0)) == 0 and n(*args(Nq=0)) == 0  # empty launches
    assert n(*args(Nip=0)) == 1 and n(*args(Nip=65)) == 1
    assert n(*args(ldq=72)) == 1      # row stride smaller than H*D
    assert n(*args(ldq=84)) == 1      # not a multiple of 8
    assert n(*args(Q=a + 2)) == 1     # alignment
    assert n(*args(ldvtip=0)) == 1    # must cover Nip rounded up to 8
    assert n(*args(sc=None)) == 1 and n(*args(idx=-1)) == 1
    assert n(*args(D=16)) == 3 and n(*args(dtype=0)) == 3  # not instantiated / float32 is composed
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------------------
# routes
# ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("D", [40, 64, 160])
def test_fused_and_composed_routes_agree(D, dtype):
    from gm_diffusion import hip_ops as ops

    B, H, Nq, Nk, Nip = 2, 2, 161, 77, 8
    scale = D ** -0.5
    q, k, v, kip, vip = R.make_qkv(B, H, Nq, Nk, Nip, D, dtype, seed=D)
    qb, kb, kipb = _rows(q, H * D, 0), _rows(k, H * D, 0), _rows(kip, H * D, 0)
    vtb, vtipb = _vt(v, _pad8(Nk)), _vt(vip, _pad8(Nip))
    sc = _scales(0.6, 2)
    fused = ops.attention_ip(qb, kb, vtb, kipb, vtipb, H, Nk, Nip, scale, sc, 2, fused=True)
    comp = ops.attention_ip(qb, kb, vtb, kipb, vtipb, H, Nk, Nip, scale, sc, 2, fused=False)
    torch.cuda.synchronize()
    dev = lambda *ts: [t.to(DEV) for t in ts]
    ref, b_f = R.decoupled_bound(*dev(q, k, v, kip, vip), scale, 0.6, dtype)
    _, b_c = R.composed_bound(*dev(q, k, v, kip, vip), scale, 0.6, dtype)
    as_heads = lambda o: o.view(B, Nq, H, D).permute(0, 2, 1, 3)
    P.assert_elementwise(as_heads(comp), ref, b_c, f"composed route D={D} {dtype}")
    P.assert_elementwise(as_heads(fused), as_heads(comp).double(), b_f + b_c, f"fused vs composed D={D} {dtype}")
    assert ops.USE_ATTN_IP_FUSED  # the default route of the 16-bit types is the fused kernel


@pytest.mark.parametrize("mode", ["split", "exact"])
def test_float32_composed_routes(mode):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion.components.unet_2d_condition import composed_attention

    B, H, Nq, Nk, Nip, D = 2, 2, 161, 77, 8, 40
    scale = D ** -0.5
    q, k, v, kip, vip = R.make_qkv(B, H, Nq, Nk, Nip, D, F32, seed=3)
    qb, kb, kipb = _rows(q, H * D, 0), _rows(k, H * D, 0), _rows(kip, H * D, 0)
    pad4 = lambda n: (n + 3) // 4 * 4
    vtb, vtipb = _vt(v, pad4(Nk)), _vt(vip, pad4(Nip))
    sc = _scales(-0.5, 15)
    prev = ops.set_f32_mode(mode)
    try:
        if mode == "split":
            got = ops.attention_ip(qb, kb, vtb, kipb, vtipb, H, Nk, Nip, scale, sc, 15)
            ref, bound = R.split_composed_bound(*[t.to(DEV) for t in (q, k, v, kip, vip)], scale, -0.5)
        else:
            a = composed_attention(qb, 0, H * D, kb, 0, H * D, vtb, B, H, D, Nq, Nk, scale, F32)
            b = composed_attention(qb, 0, H * D, kipb, 0, H * D, vtipb, B, H, D, Nq, Nip, scale, F32)
            got = ops.scaled_add(a, b, sc, 15, out=a)
            ref, bound = R.exact_composed_bound(*[t.to(DEV) for t in (q, k, v, kip, vip)], scale, -0.5)
    finally:
        ops.set_f32_mode(prev)
    torch.cuda.synchronize()
    assert not ops.is_asplit(got)
    P.assert_elementwise(got.view(B, Nq, H, D).permute(0, 2, 1, 3), ref, bound, f"float32 {mode} composed route")


@pytest.mark.parametrize("dtype", [F32, BF16, F16])
def test_scaled_add_every_dtype_and_a_second_lap(dtype):
    from gm_diffusion import hip_ops as ops

    n = 256 * 16 * 256 * 8 + 4096  # more 16-byte vectors than one pass of the largest grid: the grid-stride loop takes a second lap
    g = torch.Generator().manual_seed(4)
    a, b = torch.randn(n, generator=g).to(dtype).to(DEV), torch.randn(n, generator=g).to(dtype).to(DEV)
    sc = _scales(0.3, 7)
    got = ops.scaled_add(a, b, sc, 7)
    torch.cuda.synchronize()
    ref = a.double() + b.double() * float(torch.tensor(0.3, dtype=torch.float32))
    u = P.unit_roundoff(dtype)
    bound = 2 * P.U_F32 * (a.double().abs() + 0.3 * b.double().abs()) + u * ref.abs() * (1 + 2 * P.U_F32) + P._TINY[dtype]
    P.assert_elementwise(got, ref, bound, f"scaled_add {dtype}")


# ---------------------------------------------------------------------------------------------------------------------------
# UNet (tiny config, 16 x 16 latents, batch 2)
# ---------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _refs():
    from oracle import fixtures, unet as OU

    ou, og = fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8)
    sd = R.make_state_dict(OU.tiny_unet_config(4), tokens=4, clip_dim=32, seed=7, gain=2.0)
    return ou, og, sd


def _hip_unet(ou, dtype):
    from gm_diffusion.components import UNet2DConditionModel

    m = UNet2DConditionModel(**vars(ou.config))
    m.load_state_dict(ou.state_dict())
    return m.to(DEV, dtype)


@functools.lru_cache(maxsize=None)
def _unet_case():
    """Inputs and the CPU references, computed once: [negative; positive] rows of one latent pair (so cfg_shared applies)."""
    ou, _, sd = _refs()
    g = torch.Generator().manual_seed(61)
    lat, ctx = torch.randn(1, 4, 16, 16, generator=g), torch.randn(2, 77, 64, generator=g)
    img = torch.cat([torch.zeros(1, 2, 32), torch.randn(1, 2, 32, generator=g)])  # two images: 8 image keys; zeros = the negative
    x = torch.cat([lat, lat])
    with torch.no_grad():
        ref = R.IPAdapterRef(ou, sd, scale=0.6)
        ref.set_image_embeds(img)
        eps = ref(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
        plain = ou(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
    return lat, ctx, img, eps, plain


@pytest.mark.parametrize("dtype,mode", [(F32, "split"), (F32, "exact"), (BF16, "split"), (F16, "split")])
def test_unet_with_adapter_against_the_reference(dtype, mode):
    from gm_diffusion import hip_ops as ops

    prev = ops.set_f32_mode(mode)
    try:
        ou, _, sd = _refs()
        lat, ctx, img, eps, plain = _unet_case()
        tol = MODEL_TOL[dtype]
        hu, never = _hip_unet(ou, dtype), _hip_unet(ou, dtype)
        dlat, dctx, dimg = lat.to(DEV), ctx.to(DEV), img.to(DEV)
        dx = torch.cat([dlat, dlat])
        base = never(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        hu.load_ip_adapter(sd)
        hu.set_ip_adapter_scale(0.6)
        got = hu(dx, 501, encoder_hidden_states=dctx, added_cond_kwargs={"image_embeds": [dimg]}, return_dict=False)[0]
        e = rel_err(got, eps)
        print(f"UNet + IP-Adapter {dtype} {mode}: rel err vs the reference {e:.3e} (tol {tol:.0e}); the image prompt moves the output by "
              f"{rel_err(got, base):.3f}")
        assert got.shape == eps.shape and e < tol, e
        assert rel_err(got, base) > 10 * tol and rel_err(eps, plain) > 10 * tol  # the image prompt matters, far beyond the tolerance
        # packed: eager == graph replay, cfg_shared on == off, bit for bit
        c = hu.prepare_context(dctx)
        hu.set_timestep(501)
        ip = hu.prepare_ip_context(dimg)
        assert ip.rows == 2 and ip.nip == 8
        assert hu.prepare_ip_context(dimg) is ip  # the same tensor again: nothing is recomputed (as the text K / V^T cache)
        other = dimg.clone()
        ip2 = hu.prepare_ip_context(other)
        other.mul_(0.5)  # changed in place: prepared again, into the same persistent buffers
        assert ip2 is not ip and hu.prepare_ip_context(other) is not ip2
        ip = hu.prepare_ip_context(dimg)
        full = hu.forward_packed(hu.pack_input(dlat, dup=2), 2, 16, 16, c, ip=ip)
        assert torch.equal(full, got)
        shared = hu.forward_packed(hu.pack_input(dlat, dup=1), 2, 16, 16, c, cfg_shared=True, ip=ip)
        assert torch.equal(shared, full)
        for cs in (False, True):
            gph = hu.graphed_forward(2, 16, 16, c, cfg_shared=cs, ip=ip)
            hu.pack_input(dlat, dup=1 if cs else 2, out=gph.x)
            assert torch.equal(gph.replay(), full), f"graph replay cfg_shared={cs}"
        # the scale lives in device memory: the same graph, another value, no capture
        n_graphs = len(hu._graphs)
        hu.set_ip_adapter_scale(0.0)
        assert hu.graphed_forward(2, 16, 16, c, cfg_shared=True, ip=ip) is gph and len(hu._graphs) == n_graphs
        zero = gph.replay().clone()
        assert rel_err(zero, base) < tol and not torch.equal(zero, full)
        # a graph captured without the image prompt is another graph, and launches what it always launched
        g0 = hu.graphed_forward(2, 16, 16, c, cfg_shared=True)
        assert g0 is not gph
        hu.pack_input(dlat, dup=1, out=g0.x)
        assert torch.equal(g0.replay(), base)
        # a missing buffer during capture is an error, not an allocation inside the graph
        from gm_diffusion._native import HipExtensionError

        hu._capturing = True
        try:
            with pytest.raises(HipExtensionError):
                hu.prepare_ip_context(dimg[:1])
        finally:
            hu._capturing = False
        # unloaded: bit-identical to a UNet that never had an adapter
        hu.unload_ip_adapter()
        assert torch.equal(hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0], base)
        with pytest.raises(ValueError):
            hu(dx, 501, encoder_hidden_states=dctx, added_cond_kwargs={"image_embeds": [dimg]}, return_dict=False)
    finally:
        ops.set_f32_mode(prev)


def test_without_an_adapter_the_cross_attention_launches_are_unchanged():
    """No adapter, or an adapter and no image prompt: not one launch of the decoupled attention or the scaled add."""
    from gm_diffusion import hip_ops as ops

    ou, _, sd = _refs()
    lat, ctx, img, _, _ = _unet_case()
    hu = _hip_unet(ou, BF16)
    dx, dctx = torch.cat([lat, lat]).to(DEV), ctx.to(DEV)
    calls = {"ip": 0, "add": 0}
    real_ip, real_add = ops.attention_ip, ops.scaled_add
    ops.attention_ip = lambda *a, **k: (calls.__setitem__("ip", calls["ip"] + 1), real_ip(*a, **k))[1]
    ops.scaled_add = lambda *a, **k: (calls.__setitem__("add", calls["add"] + 1), real_add(*a, **k))[1]
    try:
        base = hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        hu.load_ip_adapter(sd)
        again = hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        assert calls == {"ip": 0, "add": 0} and torch.equal(again, base)
        hu(dx, 501, encoder_hidden_states=dctx, added_cond_kwargs={"image_embeds": [img.to(DEV)]}, return_dict=False)
        assert calls == {"ip": 16, "add": 0}  # the sixteen cross-attentions (the tiny UNet has SD-1.5's block structure), one launch each
    finally:
        ops.attention_ip, ops.scaled_add = real_ip, real_add


# ---------------------------------------------------------------------------------------------------------------------------
# pipeline (dual tiny, 2 prompts, 4 PNDM steps, 64 x 64)
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = 4
# latent RMS (sdr, gm) of the 16-bit runs against the float32 run, measured on the MI355X (printed by
# test_pipeline_16bit_against_the_float32_run): the gate is 2x these
MEASURED_16BIT_RMS = {BF16: (6.042e-2, 1.673e-2), F16: (7.649e-3, 1.867e-3)}


def _pndm():
    from gm_diffusion.components import PNDMScheduler

    return PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True, steps_offset=1,
                         set_alpha_to_one=False)


def _pipe(dtype, adapter=True, controlnet=None):
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    ou, og, sd = _refs()
    pipe = StableDiffusionDualUNetPipeline(vae=None, text_encoder=None, tokenizer=None, unet=_hip_unet(ou, dtype), gm_unet=_hip_unet(og, dtype),
                                           scheduler=_pndm(), safety_checker=None, feature_extractor=None, requires_safety_checker=False,
                                           controlnet=controlnet)
    pipe.set_progress_bar_config(disable=True)
    if adapter:
        pipe.load_ip_adapter(sd)
    return pipe


@functools.lru_cache(maxsize=None)
def _pipe_inputs():
    from oracle import fixtures

    pos, neg, lat = fixtures.make_inputs(2, 8, 8, cross_dim=64)
    img = torch.randn(1, 1, 32, generator=torch.Generator().manual_seed(8))
    return pos, neg, lat, torch.cat([torch.zeros_like(img), img])  # ip_adapter_image_embeds: [negative; positive] of ONE picture


def _kw(image=True, **extra):
    pos, neg, lat, img = _pipe_inputs()
    kw = dict(prompt_embeds=pos.to(DEV), negative_prompt_embeds=neg.to(DEV), latents=lat.to(DEV), height=64, width=64,
              num_inference_steps=STEPS, guidance_scale=7.5, output_type="latent", **extra)
    if image:
        kw["ip_adapter_image_embeds"] = [img.to(DEV)]
    return kw


@functools.lru_cache(maxsize=None)
def _ref_loop(ip_scale=1.0):
    from oracle import schedulers as osched

    ou, og, sd = _refs()
    pos, neg, lat, img = _pipe_inputs()
    rows = torch.cat([img[:1]] * 2 + [img[1:]] * 2)  # what the pipeline makes of it for two prompts under guidance
    if ip_scale is None:
        from oracle import pipelines as OP

        return OP.dual_loop(ou, og, osched.PNDMScheduler(), pos, neg, lat, num_inference_steps=STEPS, guidance_scale=7.5)
    return R.dual_loop_ip_adapter(ou, og, sd, osched.PNDMScheduler(), pos, neg, lat, rows, num_inference_steps=STEPS, guidance_scale=7.5,
                                  ip_scale=ip_scale)


@functools.lru_cache(maxsize=None)
def _f32_run():
    sdr, gm = _pipe(F32)(**_kw())
    torch.cuda.synchronize()
    return sdr.cpu(), gm.cpu()


@pytest.mark.parametrize("mode", ["split", "exact"])
def test_pipeline_f32_against_the_restated_cpu_loop(mode):
    from gm_diffusion import hip_ops as ops

    prev = ops.set_f32_mode(mode)
    try:
        pipe = _pipe(F32)
        sdr, gm = pipe(**_kw())
        ref_sdr, ref_gm = _ref_loop()
        e_sdr, e_gm = rms(sdr, ref_sdr), rms(gm, ref_gm)
        print(f"IP-Adapter pipeline float32 {mode}: latent RMS vs the CPU loop sdr={e_sdr:.3e} gm={e_gm:.3e}")
        assert e_sdr <= 1e-3 and e_gm <= 1e-3
        plain_sdr, _ = _ref_loop(ip_scale=None)
        assert rms(ref_sdr, plain_sdr) > 1e-2  # the image prompt moves the result by far more than the gate
        # the generic (non-fused) loop through the public __call__s: added_cond_kwargs = {"image_embeds": [...]}
        pipe._use_fused = lambda *args: False
        sdr2, gm2 = pipe(**_kw())
        assert rms(sdr2, ref_sdr) <= 1e-3 and rms(gm2, ref_gm) <= 1e-3
        # another scale between two calls: the reference at that scale; scale 0: the reference without an image prompt
        del pipe._use_fused
        pipe.set_ip_adapter_scale(0.5)
        sdr3, gm3 = pipe(**_kw())
        r3 = _ref_loop(ip_scale=0.5)
        assert rms(sdr3, r3[0]) <= 1e-3 and rms(gm3, r3[1]) <= 1e-3 and rms(r3[0], ref_sdr) > 1e-2
        pipe.set_ip_adapter_scale(0.0)
        sdr0, _ = pipe(**_kw())
        assert rms(sdr0, plain_sdr) <= 1e-3
    finally:
        ops.set_f32_mode(prev)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_pipeline_16bit_against_the_float32_run(dtype):
    """Measured on the MI355X (latent RMS against this project's float32 run of the same call: two prompts, 4 PNDM steps, 64 x 64,
    adapter gain 2, scale 1): bfloat16 sdr 6.042e-2 / gm 1.673e-2, float16 sdr 7.649e-3 / gm 1.867e-3 (MEASURED_16BIT_RMS); gated at
    twice the measured value.  The float32 runs sit at 5.5e-6 / 1.6e-6 of the restated CPU loop."""
    f_sdr, f_gm = _f32_run()
    sdr, gm = _pipe(dtype)(**_kw())
    e_sdr, e_gm = rms(sdr, f_sdr), rms(gm, f_gm)
    print(f"IP-Adapter pipeline {dtype}: latent RMS vs the float32 run sdr={e_sdr:.4e} gm={e_gm:.4e}")
    m_sdr, m_gm = MEASURED_16BIT_RMS[dtype]
    assert e_sdr <= 2 * m_sdr and e_gm <= 2 * m_gm


def test_pipeline_graphs_and_streams_equal_eager_and_the_scale_needs_no_capture():
    pipe = _pipe(BF16)
    pipe.co_run_plans = True  # one plan family for every mode
    pipe.use_hip_graphs, pipe.overlap_streams = False, False
    a = pipe(**_kw())
    pipe.use_hip_graphs, pipe.overlap_streams = True, True
    b = pipe(**_kw())
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    counts = (len(pipe.unet._graphs), len(pipe.gm_unet._graphs))
    pipe.set_ip_adapter_scale(0.3)
    c = pipe(**_kw())
    torch.cuda.synchronize()
    assert (len(pipe.unet._graphs), len(pipe.gm_unet._graphs)) == counts  # no new capture
    assert not torch.equal(c[0], b[0])
    pipe.use_hip_graphs, pipe.overlap_streams = False, False
    d = pipe(**_kw())
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


def test_pipeline_gm_unet_is_prompted_only_with_its_own_adapter():
    from oracle import unet as OU

    pipe = _pipe(BF16)
    a = pipe(**_kw())
    assert not pipe.gm_unet.has_ip_adapter
    pipe.gm_unet.load_ip_adapter(R.make_state_dict(OU.tiny_unet_config(8), 4, 32, seed=13, gain=2.0))
    b = pipe(**_kw())
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])  # the SDR latents are the same, the GM latents moved


def test_pipeline_controlnet_and_ip_adapter_together():
    import controlnet_ref as CR
    from gm_diffusion.components import ControlNetModel

    torch.manual_seed(5)
    cn_ref = CR.ControlNetRef(**CR.tiny_controlnet_config()).eval().requires_grad_(False)
    cn = ControlNetModel(**CR.tiny_controlnet_config())
    cn.load_state_dict(cn_ref.state_dict())
    pipe = _pipe(BF16, controlnet=cn.to(DEV, BF16))
    img = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(8)).to(DEV)
    both = pipe(**_kw(control_image=img))
    only_cn = pipe(**_kw(image=False, control_image=img))
    only_ip = pipe(**_kw(control_image=img, controlnet_conditioning_scale=0.0))
    neither = pipe(**_kw(image=False, control_image=img, controlnet_conditioning_scale=0.0))
    torch.cuda.synchronize()
    # each conditioning moves the result by far more than the 1e-3 gate of the float32 runs, alone and on top of the other
    for x, y in ((both, only_cn), (both, only_ip), (only_cn, neither), (only_ip, neither)):
        assert rms(x[0], y[0]) > 1e-2
    # and eager launches equal the captured two-stream run (above) with both conditionings on, bit for bit
    pipe.use_hip_graphs, pipe.overlap_streams, pipe.co_run_plans = False, False, True
    e = pipe(**_kw(control_image=img))
    torch.cuda.synchronize()
    assert torch.equal(e[0], both[0]) and torch.equal(e[1], both[1])
