"""GPU: LoRA adapters applied at run time.  The fused rank-update kernel (gmd_lora_update) per element against float64 and the derived
bound of tests/lora_ref.py; its write footprint, row independence, the device-resident scale; the composed routes; the adapted UNet
against the merged oracle; the pipelines against the CPU loop run with the merged oracle UNet."""
import functools
import itertools

import pytest
import torch

import lora_ref as R
import parity as P

pytestmark = pytest.mark.gpu
DEV = "cuda"
BF16, F16, F32 = torch.bfloat16, torch.float16, torch.float32
MODEL_TOL = {F32: 2e-5, BF16: 3e-2, F16: 4e-3}  # tests/test_models_gpu.py: the tiny UNet against the oracle, per dtype
CANARY = 1234.0  # exactly representable in both 16-bit types; nothing the updates produce


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


def _operands(M, K, rank, N, dtype, seed):
    """x [M, K], the factors zero-padded to a multiple of 32, y0 [M, N] (CPU, values of ``dtype``)."""
    g = torch.Generator().manual_seed(seed)
    rp = _pad(rank, 32)
    x = torch.randn(M, K, generator=g).to(dtype)
    a, b = torch.zeros(rp, K), torch.zeros(N, rp)
    a[:rank] = torch.randn(rank, K, generator=g) / K ** 0.5
    b[:, :rank] = torch.randn(N, rank, generator=g) / rank ** 0.5
    y0 = torch.randn(M, N, generator=g).to(dtype)
    return x, a.to(dtype), b.to(dtype), y0


def _call(x, a, b, ybuf, yptr_off, M, N, ldy, sc, idx, trans=None, strideY=0):
    """gmd_lora_update through the C ABI; returns the status."""
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import lib

    batch, tokens = trans if trans else (1, M)
    return lib().gmd_lora_update(x.data_ptr(), a.data_ptr(), b.data_ptr(), ybuf.data_ptr() + yptr_off * ybuf.element_size(),
                                 ops.dtype_code(x.dtype), M, x.shape[1], a.shape[0], N, x.shape[1], ldy, int(trans is not None), batch, tokens,
                                 strideY, sc.data_ptr(), idx, torch.cuda.current_stream().cuda_stream)


def _run_plain(x, a, b, y0, ldy, col, sc, idx, extra_rows=0):
    """y0 embedded at columns [col, col + N) of a canary-filled [M + extra_rows, ldy] buffer; returns the buffer after the launch."""
    from gm_diffusion._native import check

    M, N = y0.shape
    buf = torch.full((M + extra_rows, ldy), CANARY, dtype=y0.dtype)
    buf[:M, col:col + N] = y0
    buf = buf.to(DEV)
    check(_call(x.to(DEV), a.to(DEV), b.to(DEV), buf, col, M, N, ldy, sc, idx), "gmd_lora_update")
    torch.cuda.synchronize()
    return buf.cpu()


def _run_trans(x, a, b, y0, batch, tokens, ldy, sc, idx):
    """y0 [M, N] as V^T [batch, N, ldy] with canary pad columns [tokens, ldy); returns the buffer after the launch."""
    from gm_diffusion._native import check

    M, N = y0.shape
    buf = torch.full((batch, N, ldy), CANARY, dtype=y0.dtype)
    buf[:, :, :tokens] = y0.view(batch, tokens, N).permute(0, 2, 1)
    buf = buf.to(DEV)
    check(_call(x.to(DEV), a.to(DEV), b.to(DEV), buf, 0, M, N, ldy, sc, idx, trans=(batch, tokens), strideY=N * ldy), "gmd_lora_update")
    torch.cuda.synchronize()
    return buf.cpu()


# ---------------------------------------------------------------------------------------------------------------------------
# kernel, per element: a pairwise-covering table
# ---------------------------------------------------------------------------------------------------------------------------
MS, KS, RANKS, NS, WIDE, INDEX = (1, 63, 64, 161, 1030), (64, 128, 320), (1, 3, 8, 16, 64, 128), (64, 200, 320), (False, True), (0, 5)
TRANS = ((1, 77), (3, 77), (2, 130))


def _pairwise(axes):
    """Greedy pairwise cover of the product of ``axes`` (deterministic): every pair of values of two different axes meets once."""
    need = {(i, u, j, v) for i, j in itertools.combinations(range(len(axes)), 2) for u in axes[i] for v in axes[j]}
    rows, combos = [], list(itertools.product(*axes))
    while need:
        best = max(combos, key=lambda c: sum((i, c[i], j, c[j]) in need for i, j in itertools.combinations(range(len(axes)), 2)))
        need -= {(i, best[i], j, best[j]) for i, j in itertools.combinations(range(len(axes)), 2)}
        rows.append(best)
    return rows


PLAIN_CASES = _pairwise((MS, KS, RANKS, NS, WIDE, INDEX))
TRANS_CASES = _pairwise((TRANS, KS, RANKS, NS, INDEX))


def test_case_tables_are_pairwise_covering():
    for cases, axes in ((PLAIN_CASES, (MS, KS, RANKS, NS, WIDE, INDEX)), (TRANS_CASES, (TRANS, KS, RANKS, NS, INDEX))):
        for i, j in itertools.combinations(range(len(axes)), 2):
            assert {(c[i], c[j]) for c in cases} == set(itertools.product(axes[i], axes[j]))
    assert len(PLAIN_CASES) <= 48 and len(TRANS_CASES) <= 30


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_kernel_plain_per_element_zero_violations(dtype):
    """M x K x rank x N x ldy (N, or N + 320 with the window at column 160) x index, pairwise covering; scales 0.7 / -1.3 alternate."""
    worst = 0.0
    for c, (M, K, rank, N, wide, idx) in enumerate(PLAIN_CASES):
        s = (0.7, -1.3)[c % 2]
        x, a, b, y0 = _operands(M, K, rank, N, dtype, seed=100 + c)
        ldy, col = (N + 320, 160) if wide else (N, 0)
        out = _run_plain(x, a, b, y0, ldy, col, _scales(s, idx), idx)
        ref, bound = R.update_ref_bound(x, a, b, y0, torch.tensor(s, dtype=F32), dtype)
        worst = max(worst, P.assert_elementwise(out[:, col:col + N], ref, bound, f"lora_update {dtype} M={M} K={K} r={rank} N={N} ldy={ldy} "
                                                f"idx={idx}", tile=(16, 64)))
        if wide:
            assert bool((out[:, :col] == CANARY).all()) and bool((out[:, col + N:] == CANARY).all()), "columns outside [col, col + N) changed"
    print(f"lora_update plain {dtype}: {len(PLAIN_CASES)} cases, max |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_kernel_transposed_per_element_zero_violations(dtype):
    """(batch, tokens) x K x rank x N x index, pairwise covering; Y is V^T [batch, N, tokens padded to 8]."""
    worst = 0.0
    for c, ((batch, tokens), K, rank, N, idx) in enumerate(TRANS_CASES):
        s = (0.7, -1.3)[c % 2]
        M, ldy = batch * tokens, _pad(tokens, 8)
        x, a, b, y0 = _operands(M, K, rank, N, dtype, seed=500 + c)
        out = _run_trans(x, a, b, y0, batch, tokens, ldy, _scales(s, idx), idx)
        ref, bound = R.update_ref_bound(x, a, b, y0, torch.tensor(s, dtype=F32), dtype)
        got = out[:, :, :tokens].permute(0, 2, 1).reshape(M, N)
        worst = max(worst, P.assert_elementwise(got, ref, bound, f"lora_update^T {dtype} batch={batch} tokens={tokens} K={K} r={rank} N={N} "
                                                f"idx={idx}", tile=(64, 16)))
        assert bool((out[:, :, tokens:] == CANARY).all()), "pad columns [tokens, ldy) changed"
    print(f"lora_update transposed {dtype}: {len(TRANS_CASES)} cases, max |err| / bound = {worst:.3f}")


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_write_footprint(dtype):
    """Y inside a canary-filled buffer: plain mode columns [N, ldy) and the rows from M on, transposed mode tokens [tokens, ldy), keep
    their bits; every element of the target changes (|update| >> 0 with these operands) -- none is skipped."""
    M, K, rank, N = 161, 128, 8, 200
    x, a, b, y0 = _operands(M, K, rank, N, dtype, seed=9)
    out = _run_plain(x, a, b, y0, N + 320, 160, _scales(1.0, 0), 0, extra_rows=70)
    assert bool((out[M:] == CANARY).all()) and bool((out[:M, :160] == CANARY).all()) and bool((out[:M, 160 + N:] == CANARY).all())
    assert float((out[:M, 160:160 + N] != y0).double().mean()) > 0.9
    batch, tokens = 3, 77
    x, a, b, y0 = _operands(batch * tokens, K, rank, N, dtype, seed=10)
    outt = _run_trans(x, a, b, y0, batch, tokens, 80 + 16, _scales(1.0, 0), 0)
    assert bool((outt[:, :, tokens:] == CANARY).all())
    assert float((outt[:, :, :tokens].permute(0, 2, 1).reshape(-1, N) != y0).double().mean()) > 0.9


def _tiles_per_workgroup(row_blocks, N):
    """N tiles (64 columns) one workgroup walks: the host's split of csrc/lora.hip restated -- N is split over gridDim.y only as far
    as ceil(512 / row blocks), so launches with many row blocks walk several tiles per workgroup (the SD-1.5 shapes: 5 at
    32768 x 320, 3 at 8192 x 640, 2 at 2048 x 1280), launches with few walk one."""
    ntiles = _pad(N, 64) // 64
    nsplit = max(1, min(ntiles, -(-512 // row_blocks)))
    return -(-ntiles // nsplit)


# (M, K, rank, N): more than 128 row blocks, so a workgroup walks 2 (splits of 2 + 2 + 1 tiles) and 3 (3 + 3, the last tile 8 columns
# wide) N tiles: the Bw tile prefetched into registers under the MFMAs of the tile before, and the stage reused tile after tile
MULTI_TILE_PLAIN = ((8259, 64, 8, 320), (16515, 128, 3, 328))
# ((batch, tokens), K, rank, N): 210 and 258 row blocks, 2 tiles per workgroup
MULTI_TILE_TRANS = (((70, 130), 64, 8, 320), ((129, 77), 128, 16, 200))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_kernel_several_n_tiles_per_workgroup(dtype):
    """The walk over N inside one workgroup (the path of every SD-1.5 shape), per element, plain and transposed."""
    for c, (M, K, rank, N) in enumerate(MULTI_TILE_PLAIN):
        assert _tiles_per_workgroup(_pad(M, 64) // 64, N) == (2, 3)[c]
        x, a, b, y0 = _operands(M, K, rank, N, dtype, seed=700 + c)
        out = _run_plain(x, a, b, y0, N + 64, 32, _scales(0.7, 5), 5)
        ref, bound = R.update_ref_bound(x, a, b, y0, torch.tensor(0.7, dtype=F32), dtype)
        P.assert_elementwise(out[:, 32:32 + N], ref, bound, f"lora_update {dtype} M={M} K={K} r={rank} N={N}, several tiles", tile=(16, 64))
        assert bool((out[:, :32] == CANARY).all()) and bool((out[:, 32 + N:] == CANARY).all())
    for c, ((batch, tokens), K, rank, N) in enumerate(MULTI_TILE_TRANS):
        assert _tiles_per_workgroup(batch * (_pad(tokens, 64) // 64), N) == 2
        M, ldy = batch * tokens, _pad(tokens, 8)
        x, a, b, y0 = _operands(M, K, rank, N, dtype, seed=720 + c)
        out = _run_trans(x, a, b, y0, batch, tokens, ldy, _scales(-1.3, 0), 0)
        ref, bound = R.update_ref_bound(x, a, b, y0, torch.tensor(-1.3, dtype=F32), dtype)
        P.assert_elementwise(out[:, :, :tokens].permute(0, 2, 1).reshape(M, N), ref, bound,
                             f"lora_update^T {dtype} batch={batch} tokens={tokens} K={K} r={rank} N={N}, several tiles", tile=(64, 16))
        assert bool((out[:, :, tokens:] == CANARY).all())


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_row_independence_and_a_zero_scale(dtype):
    """A row's result is the same bits whatever else is in the launch, ACROSS DIFFERENT GRIDS: the first 64 rows of an M = 32768
    launch (512 row blocks, N not split: each workgroup walks all 5 tiles) and of an M = 1030 launch (17 row blocks x 5 splits of one
    tile) are bit-equal to an M = 64 launch of those rows (1 x 5); transposed, the first batch entry of 130 (2 tiles per workgroup)
    against a launch of that entry alone (1 tile).  scales[index] = 0 leaves Y equal."""
    K, rank, N = 320, 16, 320
    x, a, b, y0 = _operands(1030, K, rank, N, dtype, seed=21)
    sc = _scales(0.9, 5)
    big = _run_plain(x, a, b, y0, N, 0, sc, 5)
    small = _run_plain(x[:64].contiguous(), a, b, y0[:64].contiguous(), N, 0, sc, 5)
    assert torch.equal(big[:64].view(torch.int16), small.view(torch.int16))
    assert not torch.equal(big, y0)
    zero = _run_plain(x, a, b, y0, N, 0, _scales(0.0, 5), 5)
    assert torch.equal(zero, y0)
    xt, at, bt, yt = _operands(3 * 77, K, rank, N, dtype, seed=22)
    zt = _run_trans(xt, at, bt, yt, 3, 77, 80, _scales(0.0, 0), 0)
    assert torch.equal(zt[:, :, :77].permute(0, 2, 1).reshape(-1, N), yt)
    # different tiles per workgroup: 5 against 1 (plain), 2 against 1 (transposed)
    assert _tiles_per_workgroup(512, N) == 5 and _tiles_per_workgroup(17, N) == 1 and _tiles_per_workgroup(1, N) == 1
    xl, al, bl, yl = _operands(32768, 64, rank, N, dtype, seed=23)
    huge = _run_plain(xl, al, bl, yl, N, 0, sc, 5)
    one = _run_plain(xl[:64].contiguous(), al, bl, yl[:64].contiguous(), N, 0, sc, 5)
    assert torch.equal(huge[:64].view(torch.int16), one.view(torch.int16)) and not torch.equal(one, yl[:64])
    assert _tiles_per_workgroup(130, N) == 2
    xb, ab, bb, yb = _operands(130 * 64, 64, rank, N, dtype, seed=24)
    many = _run_trans(xb, ab, bb, yb, 130, 64, 64, sc, 5)
    first = _run_trans(xb[:64].contiguous(), ab, bb, yb[:64].contiguous(), 1, 64, 64, sc, 5)
    assert torch.equal(many[:1].view(torch.int16), first.view(torch.int16))


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_one_graph_serves_every_scale(dtype):
    from gm_diffusion import hip_ops as ops

    M, K, rank, N = 161, 128, 8, 200
    x, a, b, y0 = _operands(M, K, rank, N, dtype, seed=31)
    dx, da, db, dy0 = (t.to(DEV) for t in (x, a, b, y0))
    sc = torch.zeros(7, dtype=F32, device=DEV)
    sc[5] = 0.5
    y = dy0.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        ops.lora_update(dx, da, db, y, sc, 5, fused=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        y.copy_(dy0)
        ops.lora_update(dx, da, db, y, sc, 5, fused=True)
    for s in (0.5, -1.25, 0.0):
        sc[5] = s
        g.replay()
        torch.cuda.synchronize()
        ref, bound = R.update_ref_bound(x, a, b, y0, torch.tensor(s, dtype=F32), dtype)
        P.assert_elementwise(y.cpu(), ref, bound, f"replay at scale {s} {dtype}")


def test_argument_checks_and_empty_launches():
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import HipExtensionError, lib

    buf = torch.zeros(1 << 16, dtype=BF16, device=DEV)
    p, es = buf.data_ptr(), 2
    X, A, B_, Y = p, p + 16384 * es, p + 32768 * es, p + 49152 * es
    sc = _scales(1.0, 0)
    n = lib().gmd_lora_update

    def args(**o):
        return [o.get("X", X), A, B_, o.get("Y", Y), o.get("dtype", 1), o.get("M", 8), o.get("K", 64), o.get("Rp", 32), o.get("N", 64),
                o.get("ldx", 64), o.get("ldy", 64), o.get("trans", 0), o.get("batch", 1), o.get("tokens", 8), o.get("strideY", 0),
                o.get("sc", sc.data_ptr()), o.get("idx", 0), None]

    assert n(*args()) == 0
    assert n(*args(M=0)) == 0                                        # an empty launch
    assert n(*args(K=96)) == 1 and n(*args(K=32, ldx=32)) == 1       # K % 64
    assert n(*args(Rp=16)) == 1 and n(*args(Rp=48)) == 1             # Rp % 32
    assert n(*args(Rp=160)) == 1                                     # rank above 128
    assert n(*args(sc=None)) == 1 and n(*args(idx=-1)) == 1
    assert n(*args(X=X + 2)) == 1 and n(*args(Y=Y + 2)) == 1         # alignment
    assert n(*args(ldy=56)) == 1 and n(*args(ldy=68)) == 1           # ldy < N, ldy % 8
    assert n(*args(ldx=60)) == 1
    assert n(*args(Y=X)) == 1 and n(*args(Y=X + 64 * es)) == 1       # X overlaps Y
    assert n(*args(trans=1, batch=2, tokens=8)) == 1                 # M != batch * tokens
    assert n(*args(trans=1, batch=1, tokens=8, ldy=8, strideY=64 * 8)) == 0
    assert n(*args(trans=1, batch=1, tokens=8, ldy=8, strideY=8)) == 1
    assert n(*args(dtype=0)) == 3 and n(*args(dtype=3)) == 3         # float32 / split dtypes are composed by the caller
    assert b"gmd_lora_update" in lib().gmd_last_error()
    torch.cuda.synchronize()
    with pytest.raises(HipExtensionError):
        ops.lora_update(buf[:512].view(8, 64), buf[1024:1024 + 2048].view(32, 64), buf[4096:4096 + 2048].view(64, 32),
                        torch.zeros(8, 64, dtype=F16, device=DEV), sc, 0)


@pytest.mark.parametrize("dtype", [BF16, F16])
@pytest.mark.parametrize("trans", [False, True])
def test_fused_and_composed_routes_agree(dtype, trans):
    from gm_diffusion import hip_ops as ops

    batch, tokens, K, rank, N = 3, 77, 128, 8, 200
    M = batch * tokens
    x, a, b, y0 = _operands(M, K, rank, N, dtype, seed=41)
    sc = _scales(0.6, 2)
    dx, da, db = x.to(DEV), a.to(DEV), b.to(DEV)
    if trans:
        ldy = _pad(tokens, 8)
        yt = torch.zeros(batch, N, ldy, dtype=dtype)
        yt[:, :, :tokens] = y0.view(batch, tokens, N).permute(0, 2, 1)
        f = ops.lora_update(dx, da, db, yt.to(DEV), sc, 2, transposed=True, tokens=tokens, fused=True)
        c = ops.lora_update(dx, da, db, yt.to(DEV), sc, 2, transposed=True, tokens=tokens, fused=False)
        assert bool((f[:, :, tokens:] == 0).all()) and bool((c[:, :, tokens:] == 0).all())
        f, c = (t[:, :, :tokens].permute(0, 2, 1).reshape(M, N).cpu() for t in (f, c))
    else:  # columns [64, 64 + N) of a wider buffer
        wide = torch.full((M, N + 128), CANARY, dtype=dtype)
        wide[:, 64:64 + N] = y0
        f = ops.lora_update(dx, da, db, wide.to(DEV), sc, 2, col=64, fused=True).cpu()
        c = ops.lora_update(dx, da, db, wide.to(DEV), sc, 2, col=64, fused=False).cpu()
        for t in (f, c):
            assert bool((t[:, :64] == CANARY).all()) and bool((t[:, 64 + N:] == CANARY).all())
        f, c = f[:, 64:64 + N], c[:, 64:64 + N]
    torch.cuda.synchronize()
    s = torch.tensor(0.6, dtype=F32)
    ref, b_f = R.update_ref_bound(x, a, b, y0, s, dtype)
    _, b_c = R.update_ref_bound(x, a, b, y0, s, dtype, route="composed")
    P.assert_elementwise(f, ref, b_f, f"fused {dtype} trans={trans}")
    P.assert_elementwise(c, ref, b_c, f"composed {dtype} trans={trans}")
    P.assert_elementwise(f, c.double(), b_f + b_c, f"fused vs composed {dtype} trans={trans}")
    assert ops.USE_LORA_FUSED  # the default route of the 16-bit types is the fused kernel


@pytest.mark.parametrize("mode", ["split", "exact"])
@pytest.mark.parametrize("trans", [False, True])
def test_float32_composed_route(mode, trans):
    """float32, both contraction modes, against float64; the factors prepared as the model prepares them (_wt / _wa)."""
    from gm_diffusion import hip_ops as ops

    batch, tokens, K, rank, N = 3, 77, 128, 8, 200
    M = batch * tokens
    mult = 32 if mode == "split" else 16
    g = torch.Generator().manual_seed(51)
    x, y0 = torch.randn(M, K, generator=g), torch.randn(M, N, generator=g)
    a, b = torch.zeros(_pad(rank, mult), K), torch.zeros(N, _pad(rank, mult))
    a[:rank], b[:, :rank] = torch.randn(rank, K, generator=g) / K ** 0.5, torch.randn(N, rank, generator=g) / rank ** 0.5
    sc = _scales(-0.5, 6)
    prev = ops.set_f32_mode(mode)
    try:
        assert ops.lora_rank_multiple(F32) == mult
        da = ops.split_weights(a.to(DEV)) if mode == "split" else a.to(DEV)
        if trans:
            db = ops.scale_weight(b.to(DEV)) if mode == "split" else b.to(DEV)
            ldy = _pad(tokens, 4)
            yt = torch.zeros(batch, N, ldy)
            yt[:, :, :tokens] = y0.view(batch, tokens, N).permute(0, 2, 1)
            got = ops.lora_update(x.to(DEV), da, db, yt.to(DEV), sc, 6, transposed=True, tokens=tokens)
            assert bool((got[:, :, tokens:] == 0).all())
            got = got[:, :, :tokens].permute(0, 2, 1).reshape(M, N)
        else:
            db = ops.split_weights(b.to(DEV)) if mode == "split" else b.to(DEV)
            got = ops.lora_update(x.to(DEV), da, db, y0.to(DEV), sc, 6)
        torch.cuda.synchronize()
    finally:
        ops.set_f32_mode(prev)
    ref, bound = R.update_ref_bound_f32(x, a, b, y0, torch.tensor(-0.5, dtype=F32), mode)
    P.assert_elementwise(got.cpu(), ref, bound, f"float32 {mode} trans={trans}")


# ---------------------------------------------------------------------------------------------------------------------------
# UNet (tiny config, 16 x 16 latents, batch 2)
# ---------------------------------------------------------------------------------------------------------------------------
RANK, GAIN, SEED, ALPHA = 4, 2.0, 11, 2.0


@functools.lru_cache(maxsize=None)
def _refs():
    from oracle import fixtures

    ou, og = fixtures.build_unet("tiny", 4), fixtures.build_unet("tiny", 8)
    canon = R.canonical(ou, RANK, SEED, GAIN, alpha=ALPHA)
    return ou, og, canon, R.to_convention(canon, "kohya")


def _hip_unet(ou, dtype):
    from gm_diffusion.components import UNet2DConditionModel

    m = UNet2DConditionModel(**vars(ou.config))
    m.load_state_dict(ou.state_dict())
    return m.to(DEV, dtype)


@functools.lru_cache(maxsize=None)
def _unet_case():
    """Inputs and the CPU references, computed once: [negative; positive] rows of one latent pair (so cfg_shared applies)."""
    ou, _, canon, _ = _refs()
    g = torch.Generator().manual_seed(61)
    lat, ctx = torch.randn(1, 4, 16, 16, generator=g), torch.randn(2, 77, 64, generator=g)
    x = torch.cat([lat, lat])
    with torch.no_grad():
        eps = {s: R.merged_oracle(ou, canon, s)(x, torch.tensor(501), encoder_hidden_states=ctx)[0] for s in (1.0, 0.5)}
        plain = ou(x, torch.tensor(501), encoder_hidden_states=ctx)[0]
    return lat, ctx, eps, plain


@pytest.mark.parametrize("dtype,mode", [(F32, "split"), (F32, "exact"), (BF16, "split"), (F16, "split")])
def test_unet_with_adapter_against_the_merged_oracle(dtype, mode):
    from gm_diffusion import hip_ops as ops
    from gm_diffusion._native import HipExtensionError

    prev = ops.set_f32_mode(mode)
    try:
        ou, _, _, sd = _refs()
        lat, ctx, eps, plain = _unet_case()
        tol = MODEL_TOL[dtype]
        hu, never = _hip_unet(ou, dtype), _hip_unet(ou, dtype)
        dlat, dctx = lat.to(DEV), ctx.to(DEV)
        dx = torch.cat([dlat, dlat])
        base = never(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        hu.load_lora(sd)
        got = hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        e = rel_err(got, eps[1.0])
        print(f"UNet + LoRA {dtype} {mode}: rel err vs the merged oracle {e:.3e} (tol {tol:.0e}); the adapter moves the output by "
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
        for cs in (False, True):
            gph = hu.graphed_forward(2, 16, 16, c, cfg_shared=cs)
            hu.pack_input(dlat, dup=1 if cs else 2, out=gph.x)
            assert torch.equal(gph.replay(), full), f"graph replay cfg_shared={cs}"
        # the same prompt tensor at a new scale equals a fresh model at that scale (the cross-attention K / V^T cache key), through
        # the SAME graph object: the scale lives in device memory
        n_graphs = len(hu._graphs)
        hu.set_lora_scale(0.5)
        assert hu.graphed_forward(2, 16, 16, c, cfg_shared=True) is gph and len(hu._graphs) == n_graphs
        half = gph.replay().clone()
        fresh = _hip_unet(ou, dtype)
        fresh.load_lora(sd)
        fresh.set_lora_scale(0.5)
        assert torch.equal(half, fresh(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0])
        assert rel_err(half, eps[0.5]) < tol and not torch.equal(half, full)
        hu.set_lora_scale(0.0)
        assert hu.graphed_forward(2, 16, 16, c, cfg_shared=True) is gph
        zero = gph.replay().clone()
        assert rel_err(zero, base) < tol
        hu._capturing = True
        try:
            with pytest.raises(HipExtensionError):
                hu.set_lora_scale(1.0)
        finally:
            hu._capturing = False
        # unloaded: bit-identical to a UNet that never had an adapter, and the adapter's graphs are gone
        hu.unload_lora()
        assert not hu.has_lora and not any(("lora" in str(k)) for k in hu._graphs)
        assert torch.equal(hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0], base)
        g0 = hu.graphed_forward(2, 16, 16, c, cfg_shared=True)
        hu.pack_input(dlat, dup=1, out=g0.x)
        assert torch.equal(g0.replay(), base)
    finally:
        ops.set_f32_mode(prev)


def test_update_launch_counts_with_and_without_an_adapter():
    """Without an adapter not one lora_update; with one, 8 per transformer block and forward, 2 of them only inside _cross_kv (so a
    second forward on the same prompt tensor issues 6 per block)."""
    from gm_diffusion import hip_ops as ops

    ou, _, _, sd = _refs()
    lat, ctx, _, _ = _unet_case()
    hu = _hip_unet(ou, BF16)
    dx, dctx = torch.cat([lat, lat]).to(DEV), ctx.to(DEV)
    calls = {"n": 0}
    real = ops.lora_update
    ops.lora_update = lambda *a, **k: (calls.__setitem__("n", calls["n"] + 1), real(*a, **k))[1]
    try:
        base = hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        assert calls["n"] == 0
        hu.load_lora(sd)
        c = hu.prepare_context(dctx)
        hu.set_timestep(501)
        hu.update_context(c)
        assert calls["n"] == 2 * 16
        hu.forward_packed(hu.pack_input(dx), 2, 16, 16, c)
        assert calls["n"] == 8 * 16
        hu.forward_packed(hu.pack_input(dx), 2, 16, 16, c)
        assert calls["n"] == 14 * 16
        hu.unload_lora()
        again = hu(dx, 501, encoder_hidden_states=dctx, return_dict=False)[0]
        assert calls["n"] == 14 * 16 and torch.equal(again, base)
    finally:
        ops.lora_update = real


# ---------------------------------------------------------------------------------------------------------------------------
# pipelines (dual tiny, 2 prompts, 4 PNDM steps, 64 x 64)
# ---------------------------------------------------------------------------------------------------------------------------
STEPS = 4
# latent RMS (sdr, gm) of the 16-bit runs against the float32 run, measured on the MI355X (printed by
# test_pipeline_16bit_against_the_float32_run): the gate is 2x these
MEASURED_16BIT_RMS = {BF16: (8.693e-2, 2.747e-2), F16: (1.048e-2, 3.295e-3)}


def _pndm():
    from gm_diffusion.components import PNDMScheduler

    return PNDMScheduler(beta_start=0.00085, beta_end=0.012, beta_schedule="scaled_linear", skip_prk_steps=True, steps_offset=1,
                         set_alpha_to_one=False)


def _pipe(dtype, adapter=True, controlnet=None):
    from gm_diffusion.pipelines import StableDiffusionDualUNetPipeline

    ou, og, _, sd = _refs()
    pipe = StableDiffusionDualUNetPipeline(vae=None, text_encoder=None, tokenizer=None, unet=_hip_unet(ou, dtype), gm_unet=_hip_unet(og, dtype),
                                           scheduler=_pndm(), safety_checker=None, feature_extractor=None, requires_safety_checker=False,
                                           controlnet=controlnet)
    pipe.set_progress_bar_config(disable=True)
    if adapter:
        pipe.load_lora_weights(sd)
    return pipe


def _kw(**extra):
    from oracle import fixtures

    pos, neg, lat = fixtures.make_inputs(2, 8, 8, cross_dim=64)
    return dict(prompt_embeds=pos.to(DEV), negative_prompt_embeds=neg.to(DEV), latents=lat.to(DEV), height=64, width=64,
                num_inference_steps=STEPS, guidance_scale=7.5, output_type="latent", **extra)


@functools.lru_cache(maxsize=None)
def _ref_loop(scale=1.0):
    from oracle import fixtures, pipelines as OP, schedulers as osched

    ou, og, canon, _ = _refs()
    pos, neg, lat = fixtures.make_inputs(2, 8, 8, cross_dim=64)
    unet = ou if scale is None else R.merged_oracle(ou, canon, scale)
    return OP.dual_loop(unet, og, osched.PNDMScheduler(), pos, neg, lat, num_inference_steps=STEPS, guidance_scale=7.5)


@functools.lru_cache(maxsize=None)
def _f32_run():
    sdr, gm = _pipe(F32)(**_kw())
    torch.cuda.synchronize()
    return sdr.cpu(), gm.cpu()


@pytest.mark.parametrize("mode", ["split", "exact"])
def test_pipeline_f32_against_the_cpu_loop_with_the_merged_oracle(mode):
    from gm_diffusion import hip_ops as ops

    prev = ops.set_f32_mode(mode)
    try:
        pipe = _pipe(F32)
        sdr, gm = pipe(**_kw())
        ref_sdr, ref_gm = _ref_loop()
        e_sdr, e_gm = rms(sdr, ref_sdr), rms(gm, ref_gm)
        print(f"LoRA pipeline float32 {mode}: latent RMS vs the CPU loop sdr={e_sdr:.3e} gm={e_gm:.3e}")
        assert e_sdr <= 1e-3 and e_gm <= 1e-3  # RMS_TOL of tests/test_pipeline_gpu.py
        plain_sdr, _ = _ref_loop(scale=None)
        assert rms(ref_sdr, plain_sdr) > 1e-2  # the adapter moves the result by far more than the gate
        # cross_attention_kwargs={"scale": 0.5}: the reference at that scale
        sdr5, gm5 = pipe(**_kw(cross_attention_kwargs={"scale": 0.5}))
        r5 = _ref_loop(scale=0.5)
        assert rms(sdr5, r5[0]) <= 1e-3 and rms(gm5, r5[1]) <= 1e-3 and rms(r5[0], ref_sdr) > 1e-2
    finally:
        ops.set_f32_mode(prev)


@pytest.mark.parametrize("dtype", [BF16, F16])
def test_pipeline_16bit_against_the_float32_run(dtype):
    """Measured on the MI355X (latent RMS against this project's float32 run of the same call: two prompts, 4 PNDM steps, 64 x 64,
    rank 4, gain 2, alpha 2, scale 1): bfloat16 sdr 8.693e-2 / gm 2.747e-2, float16 sdr 1.048e-2 / gm 3.295e-3 (MEASURED_16BIT_RMS);
    gated at twice the measured value.  The float32 runs sit at 1.0e-5 / 3.0e-6 of the CPU loop with the merged oracle UNet."""
    f_sdr, f_gm = _f32_run()
    sdr, gm = _pipe(dtype)(**_kw())
    e_sdr, e_gm = rms(sdr, f_sdr), rms(gm, f_gm)
    print(f"LoRA pipeline {dtype}: latent RMS vs the float32 run sdr={e_sdr:.4e} gm={e_gm:.4e}")
    m_sdr, m_gm = MEASURED_16BIT_RMS[dtype]
    assert e_sdr <= 2 * m_sdr and e_gm <= 2 * m_gm


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
    again = pipe(**_kw())  # the key held for that call only: back at the UNet's own scale, through the same graphs
    torch.cuda.synchronize()
    assert torch.equal(again[0], b[0]) and torch.equal(again[1], b[1]) and pipe.unet._lora_scale == 1.0
    assert (len(pipe.unet._graphs), len(pipe.gm_unet._graphs)) == counts
    other = _pipe(BF16)
    other.co_run_plans = True
    other.unet.set_lora_scale(0.5)
    d = other(**_kw())
    torch.cuda.synchronize()
    assert torch.equal(c[0], d[0]) and torch.equal(c[1], d[1])


def test_pipeline_gm_unet_is_adapted_only_by_its_own_load_lora():
    _, og, _, _ = _refs()
    pipe = _pipe(BF16)
    a = pipe(**_kw())
    assert pipe.unet.has_lora and not pipe.gm_unet.has_lora
    pipe.gm_unet.load_lora(R.to_convention(R.canonical(og, RANK, SEED + 1, GAIN), "peft"))
    b = pipe(**_kw())
    torch.cuda.synchronize()
    assert torch.equal(a[0], b[0]) and not torch.equal(a[1], b[1])  # the SDR latents are the same, the GM latents moved
    pipe.unload_lora_weights()
    assert not pipe.unet.has_lora and pipe.gm_unet.has_lora


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


def test_gm_pipeline_loads_and_applies_an_adapter():
    from gm_diffusion.pipelines import StableDiffusionGMPipeline

    _, og, _, _ = _refs()
    from oracle import fixtures

    pipe = StableDiffusionGMPipeline(vae=None, text_encoder=None, tokenizer=None, unet=_hip_unet(og, BF16), scheduler=_pndm(),
                                     safety_checker=None, feature_extractor=None, requires_safety_checker=False)
    pipe.set_progress_bar_config(disable=True)
    pos, neg, lat = fixtures.make_inputs(1, 8, 8, cross_dim=64)
    sdr_latent = torch.randn(1, 4, 8, 8, generator=torch.Generator().manual_seed(2)).to(DEV)
    kw = dict(prompt_embeds=pos.to(DEV), negative_prompt_embeds=neg.to(DEV), latents=lat.to(DEV), num_inference_steps=STEPS,
              guidance_scale=7.5, output_type="latent")
    plain = pipe(sdr_latent, **kw).images.clone()
    pipe.load_lora_weights(R.to_convention(R.canonical(og, RANK, SEED, GAIN), "diffusers_old"))
    adapted = pipe(sdr_latent, **kw).images.clone()
    assert rms(adapted, plain) > 1e-2
    off = pipe(sdr_latent, cross_attention_kwargs={"scale": 0.0}, **kw).images.clone()
    assert rms(off, plain) < 1e-2 and rms(off, plain) < 0.2 * rms(adapted, plain)
    pipe.unload_lora_weights()
    assert torch.equal(pipe(sdr_latent, **kw).images, plain)
