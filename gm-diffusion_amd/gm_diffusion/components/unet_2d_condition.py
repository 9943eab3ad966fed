"""
``UNet2DConditionModel`` for the MI355X build -- the denoiser the reference pipelines call at
gm_diffusion/pipelines/stable_diffusion_gm.py:1051-1059 and
stable_diffusion_dual_unet.py:1052-1060, 1083-1092:

    unet(sample, t, encoder_hidden_states=..., return_dict=False)[0]

In the reference this is ``diffusers.UNet2DConditionModel`` (un-vendored dependency) with the
SD-1.5 hyper-parameters hard-coded at scripts/inference/generate_hdr.py:116-135 and
``in_channels`` 4 (SDR UNet) or 8 (GM UNet).  Here the same network runs entirely on the
hand-written HIP kernels of libgmd_hip.so over channels-last activations:

  * conv3x3 (+bias +time-embedding +residual)      -> gmd_conv3x3 (implicit GEMM, MFMA)
  * Linear / conv1x1 (+bias +residual +SiLU)       -> gmd_gemm_nt
  * GroupNorm(+SiLU), LayerNorm, GEGLU              -> gmd_groupnorm_*, gmd_layernorm, gmd_geglu
  * self / cross attention                          -> gmd_attention (bf16) or GEMM+softmax+GEMM (f32)
  * 8-channel concat / CFG duplicate / layout+cast  -> gmd_pack_unet_input, gmd_unpack_nchw

State-dict keys follow diffusers so a real SD-1.5 checkpoint loads.
There is no CPU path: ``forward`` raises ``HipExtensionError`` off-device.

dtype policy: weights/activations are ``self.dtype`` (bfloat16 or float16 = MFMA path -- float16 is what the
reference's own half-precision scripts use, scripts/stage2/experiments/batch_size_sweep.py -- float32 = parity
path); the input latents are float32 NCHW and are cast while being packed; the output eps is
float32 NCHW taken from the fp32 accumulators of ``conv_out`` (never rounded to bf16).
"""
from __future__ import annotations

import math
import os

import torch

from .. import hip_ops as ops
from .._native import HipExtensionError
from .configuration import ConfigMixin, read_state_dict

SD15_UNET_DEFAULTS = dict(
    sample_size=64, in_channels=4, out_channels=4, center_input_sample=False, flip_sin_to_cos=True, freq_shift=0,
    down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
    up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
    block_out_channels=(320, 640, 1280, 1280), layers_per_block=2, downsample_padding=1, mid_block_scale_factor=1,
    act_fn="silu", norm_num_groups=32, norm_eps=1e-5, cross_attention_dim=768, attention_head_dim=8,
    time_cond_proj_dim=None,
    # SDXL-style options (BASELINE.json configs[4]; the reference has no such path -- SURVEY.md §7 "SDXL / fp8" -- so these
    # follow diffusers' UNet2DConditionModel config names and are checked against the oracle's restatement only): all off for SD-1.5
    transformer_layers_per_block=1, use_linear_projection=False, addition_embed_type=None, addition_time_embed_dim=None,
    projection_class_embeddings_input_dim=None,
)

# stabilityai/stable-diffusion-xl-base-1.0 unet/config.json as restated in oracle/unet.py (2,567,463,684 parameters)
SDXL_UNET_CONFIG = dict(
    block_out_channels=(320, 640, 1280), down_block_types=("DownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D"),
    up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "UpBlock2D"), transformer_layers_per_block=(1, 2, 10),
    attention_head_dim=(5, 10, 20), cross_attention_dim=2048, use_linear_projection=True, addition_embed_type="text_time",
    addition_time_embed_dim=256, projection_class_embeddings_input_dim=2816, sample_size=128,
)


def _pad_to(n, m):
    return (n + m - 1) // m * m


def _in_own_f32_mode(fn):
    """Run a module's compute method under the float32 contraction mode its weights were laid out for.  ``hip_ops`` reads the mode at
    every call, while a module's weights are pre-split / power-of-two scaled / channel-padded for ONE mode when they are placed on
    the device: a model prepared under "split" and run after ``set_f32_mode("exact")`` (bench.py holds both kinds alive) would
    otherwise run the split kernels' weights through the exact kernels or the other way round.  The override is scoped to the calling
    THREAD (``hip_ops.f32_mode_scope``): two host threads driving a "split" and an "exact" module at the same time keep their own
    modes.  16-bit modules do not depend on the mode."""
    import functools

    @functools.wraps(fn)
    def run(self, *args, **kwargs):
        self._ensure()
        if self._dtype != torch.float32 or self._f32_mode == ops.f32_mode():
            return fn(self, *args, **kwargs)
        with ops.f32_mode_scope(self._f32_mode):
            return fn(self, *args, **kwargs)

    return run


class _HipModule(ConfigMixin):
    """Shared weight handling: raw CPU float32 state-dict -> device tensors in kernel layouts."""

    def _init_module(self):
        self._raw = None       # diffusers-keyed CPU float32 tensors
        self._w = None         # prepared device tensors
        self._dtype = torch.float32
        self._device = torch.device("cpu")
        self._f32_mode = None  # float32 contraction mode the prepared weights are laid out for (set by _ensure)

    @property
    def dtype(self):
        return self._dtype

    @property
    def device(self):
        return self._device

    def state_dict(self):
        return dict(self._raw or {})

    def load_state_dict(self, sd, strict=True):
        want = self.expected_keys()
        missing = [k for k in want if k not in sd]
        unexpected = [k for k in sd if k not in want]
        if strict and (missing or unexpected):
            raise KeyError(f"{type(self).__name__}.load_state_dict: missing={missing[:5]} (+{max(len(missing) - 5, 0)}) "
                           f"unexpected={unexpected[:5]} (+{max(len(unexpected) - 5, 0)})")
        bad = [k for k in want if k in sd and tuple(sd[k].shape) != tuple(want[k])]
        if bad:
            raise ValueError(f"shape mismatch for {bad[:5]}: e.g. {tuple(sd[bad[0]].shape)} vs {tuple(want[bad[0]])}")
        self._raw = {k: sd[k].detach().to("cpu", torch.float32) for k in want if k in sd}
        self._w = None
        return self

    def to(self, *args, **kwargs):
        device, dtype = kwargs.get("device"), kwargs.get("dtype")
        for a in args:
            if isinstance(a, torch.dtype):
                dtype = a
            elif a is not None:
                device = a
        if dtype is not None:
            self._dtype = dtype
        if device is not None:
            self._device = torch.device(device)
        self._w = None
        return self

    def cuda(self):
        return self.to("cuda")

    def eval(self):
        return self

    def requires_grad_(self, flag=False):
        return self

    def _ensure(self):
        if self._w is not None:
            return
        if self._raw is None:
            raise RuntimeError(f"{type(self).__name__} has no weights: call load_state_dict()/from_pretrained() first")
        if self._device.type != "cuda":
            raise HipExtensionError(f"{type(self).__name__} runs on hand-written HIP kernels only; call .to('cuda') "
                                    "(there is no CPU fallback in the MI355X build)")
        ops.dtype_code(self._dtype)
        self._f32_mode = ops.f32_mode()  # _prepare and every later forward of this module use THIS mode (_in_own_f32_mode)
        self._w = self._prepare()

    # -- layout helpers --------------------------------------------------------------------------
    def _kmul(self):
        """Channel multiple the convolution kernels need: 64 (16-bit), 32 (float32 on the matrix cores), 16 (exact float32)."""
        return 64 if ops.is_half(self._dtype) else (32 if self._split_mode() else 16)

    def _act(self, t):
        return t.to(self._device, self._dtype).contiguous()

    def _f32(self, t):
        return t.to(self._device, torch.float32).contiguous()

    def _split_mode(self):
        """float32 module laid out for the matrix-core ("split") kernels: from the record taken when the weights were prepared."""
        return self._dtype == torch.float32 and (self._f32_mode or ops.f32_mode()) == "split"

    def _wt(self, t):
        """A weight that is the W operand of gemm_nt / conv3x3.  float32 on the matrix cores: scaled by a power of two and
        split into float16 hi / lo once, here (hip_ops.split_weights)."""
        w = self._act(t)
        if self._split_mode() and w.dim() == 2 and w.shape[1] % 32 == 0:
            return ops.split_weights(w)
        return w

    def _wa(self, t):
        """A weight that is the A operand (V^T[b] = W_v x_b^T): plain float32, power-of-two scaled in split mode."""
        w = self._act(t)
        return ops.scale_weight(w) if self._split_mode() else w

    def _conv3(self, key, cin_pad=None):
        w = self._raw[key + ".weight"]  # [Cout, Cin, 3, 3]
        cout, cin = w.shape[0], w.shape[1]
        cin_pad = cin_pad or cin
        t = torch.zeros(cout, 3, 3, cin_pad)
        t[..., :cin] = w.permute(0, 2, 3, 1)
        return self._wt(t.reshape(cout, 9 * cin_pad)), self._f32(self._raw[key + ".bias"])

    def _lin(self, key, bias=True):
        w = self._raw[key + ".weight"]
        w = w.reshape(w.shape[0], -1)  # Linear [out,in] or conv1x1 [out,in,1,1]
        return self._wt(w), (self._f32(self._raw[key + ".bias"]) if bias else None)

    def _norm(self, key):
        return self._f32(self._raw[key + ".weight"]), self._f32(self._raw[key + ".bias"])


SCORE_CHUNK_BYTES = 1 << 30  # composed_attention: float32 score matrix held at once (16,384^2 tokens = exactly this)


def composed_attention(q, q_col, ldq, k, k_col, ldk, vt, B, H, d, nq, nk, scale, dtype, causal=False):
    """Attention as GEMM -> row softmax -> GEMM (float32 parity path and the d=512 VAE block).
    q/k: buffers with rows of ldq/ldk elements, head h at columns q_col + h*d; vt: [B, H*d, ldvt] with
    zero-filled columns >= nk.  Returns [B, nq, H*d]."""
    es = q.element_size()
    mul = 64 if ops.is_half(dtype) else 4
    nkp = _pad_to(nk, mul)
    ldvt = vt.shape[2]
    if ldvt < nkp:
        raise HipExtensionError("composed_attention: vt row stride too small")
    out = torch.empty((B, nq, H * d), dtype=dtype, device=q.device)
    # the float32 scores of all heads for `rows` query rows at a time: the whole [H, nq, nkp] matrix while it stays within
    # SCORE_CHUNK_BYTES (every size up to the VAE's 16,384 tokens of a 1024 x 1024 image: one pass, as before); beyond that
    # (1920 x 1080: 32,400 tokens, 4.2 GB of scores, more than one raw buffer descriptor addresses) the query rows are walked in
    # chunks -- a row's softmax needs only its own scores, so each chunk is a complete attention over all keys
    rows = nq
    if H * nq * nkp * 4 > SCORE_CHUNK_BYTES:
        rows = max(256, SCORE_CHUNK_BYTES // (H * nkp * 4) // 256 * 256)
        if causal:
            raise HipExtensionError("composed_attention: a causal mask over chunked query rows is not implemented")
    s = torch.empty((H, min(rows, nq), nkp), dtype=torch.float32, device=q.device)
    for b in range(B):
        for r0 in range(0, nq, rows):
            nr = min(rows, nq - r0)
            sc = s if nr == s.shape[1] else s.view(-1)[:H * nr * nkp].view(H, nr, nkp)
            ops.gemm_raw(q.data_ptr() + ((b * nq + r0) * ldq + q_col) * es, k.data_ptr() + (b * nk * ldk + k_col) * es, sc.data_ptr(),
                         dtype, torch.float32, nr, nk, d, ldq, ldk, nkp, batch=H, sA=d, sW=d, sC=nr * nkp)
            p = ops.softmax_rows(sc, nk, scale, dtype, ldp=nkp, causal_nq=nq if causal else 0)
            # float32: the probabilities (~1/nk) would lose their float16 lo half to the subnormal range in a split product, so
            # this one stays on the exact kernel (small: the VAE mid block and the 77-token text encoder only)
            ops.gemm_raw(p.data_ptr(), vt.data_ptr() + b * H * d * ldvt * es, out.data_ptr() + (b * nq + r0) * H * d * es,
                         dtype, dtype, nr, d, nkp, nkp, ldvt, H * d, batch=H, sA=nr * nkp, sW=d * ldvt, sC=d, exact=True)
    return out


def _lora_layer(model, t):
    """The LoRA factors of transformer block ``t`` of ``model`` ({projection: (a, b, index)}), or None: no adapter loaded, the block
    not targeted, or a model that takes none (a ControlNet shares the UNet's block code and is not adapted)."""
    if getattr(model, "_lora_raw", None) is None:
        return None
    lw = model._lora_w
    if lw is None or model._lora_w_of is not model._w:
        raise HipExtensionError("the LoRA adapter must be prepared (update_context / a forward) before it is read")
    return lw["layers"].get(t["key"])


def _lora_key(model):
    return None if getattr(model, "_lora_raw", None) is None else (model._lora_id, model._lora_version)


class _LoraStack:
    """A projection targeted by two or more adapters: the stacked factors ``a`` [Rp, K] / ``b`` [N, Rp] and the module's ``row`` in the
    table of column scales (the one stacked launch), or ``parts`` = [(a_i, b_i, slot_i)] in load order (the sequential route: float32,
    GMD_LORA_STACK_FUSED=0).  Only the operands of the route the model takes are on the device."""

    def __init__(self, a, b, row, parts):
        self.a, self.b, self.row, self.parts = a, b, row, parts

    def seq(self, scales):
        return None if self.parts is None else [(a, b, scales, i) for a, b, i in self.parts]


def _lora_apply(model, lr, proj, x, y, col=0, tokens=None, x_split=False):
    """ONE launch behind an adapted projection -- ``hip_ops.lora_update`` for a projection one adapter targets,
    ``hip_ops.lora_update_stacked`` for one that several target (nothing when no adapter targets ``proj`` of this block)."""
    ent = lr.get(proj)
    if ent is None:
        return
    lw = model._lora_w
    if isinstance(ent, _LoraStack):
        ops.lora_update_stacked(x, ent.a, ent.b, y, lw["colscales"], ent.row, transposed=tokens is not None, tokens=tokens, col=col,
                                x_split=x_split, parts=ent.seq(lw["scales"]))
    else:
        ops.lora_update(x, ent[0], ent[1], y, lw["scales"], ent[2], transposed=tokens is not None, tokens=tokens, col=col, x_split=x_split)


_LORA_IDS = [0]


class _GraphedForward:
    """A captured UNet forward: static input ``x``, static output ``out``, ``replay()`` on the current stream."""

    x = None
    out = None
    graph = None
    ws = None

    def replay(self):
        self.graph.replay()
        return self.out


class _IPContext:
    """An image prompt prepared by ``UNet2DConditionModel.prepare_ip_context``: the row count and the number of image keys select the
    persistent K_ip / V_ip^T buffers the cross-attentions read; ``tokens`` [rows, Nip, cross_dim] are the projected IP tokens."""

    def __init__(self, rows, nip, tokens, owner):
        self.rows, self.nip, self.tokens, self.owner = rows, nip, tokens, owner


class UNet2DConditionModel(_HipModule):
    config_name = "config.json"
    max_cached_graphs = 8  # captured forwards kept per model (one per batch / latent size / token count)
    _defaults = SD15_UNET_DEFAULTS

    def __init__(self, **config):
        cfg = dict(SD15_UNET_DEFAULTS)
        unknown = [k for k in config if k not in cfg and not k.startswith("_")]
        cfg.update({k: v for k, v in config.items() if k in cfg})
        # generate_hdr.py:103-105 rewrites `num_attention_heads` to the legacy `attention_head_dim` name
        if "num_attention_heads" in config and config["num_attention_heads"] is not None:
            cfg["attention_head_dim"] = config["num_attention_heads"]
        if isinstance(cfg["attention_head_dim"], (list, tuple)) and len(set(cfg["attention_head_dim"])) == 1:
            cfg["attention_head_dim"] = cfg["attention_head_dim"][0]
        if cfg["act_fn"] != "silu" or cfg["center_input_sample"]:
            raise NotImplementedError("only silu / no centering UNets are implemented (SD-1.5, SDXL, guidance-embedded LCM)")
        tcd = cfg["time_cond_proj_dim"]
        if tcd is not None and (isinstance(tcd, bool) or not isinstance(tcd, int) or tcd <= 0):
            raise ValueError(f"time_cond_proj_dim must be a positive int or None (got {tcd!r})")
        if cfg["addition_embed_type"] not in (None, "text_time"):
            raise NotImplementedError(f"addition_embed_type={cfg['addition_embed_type']!r}")
        self._unknown_config = unknown
        self.register_to_config(**cfg)
        self._init_module()
        self._kv_cache = {}
        self._t_dev = None
        self._capturing = False
        self._transformers = []
        self._graphs = {}
        self._aug = {}  # text_time conditioning: persistent [B, temb] buffers, rewritten in place by set_added_cond
        self._tcond = {}  # time_cond_proj_dim: persistent [B, ch0] buffers of cond_proj(timestep_cond), rewritten in place by set_timestep_cond
        self._ip_raw = None       # IP-Adapter: CPU float32 weights (load_ip_adapter), None when no adapter is loaded
        self._ip_w = None         # ... the same in kernel layouts, built on first use (_ensure_ip) for the prepared weights `_ip_w_of`
        self._ip_w_of = None
        self._ip_kv = {}          # ... persistent K_ip / V_ip^T per (layer, rows, Nip, dtype), rewritten in place by prepare_ip_context
        self._ip_scale = 1.0      # ... set_ip_adapter_scale
        self._ip_last = None      # ... (key of the embeddings, their context, the embeddings) of the latest prepare_ip_context
        self._lora_adapters = {}  # LoRA: {adapter name: {module: (A [r, K], B [N, r], alpha or None)}} CPU float32, in load order (load_lora)
        self._lora_weights = {}   # ... {adapter name: weight} (set_adapters; 1.0 at load)
        self._lora_saved = None   # ... the weights disable_lora() remembered for enable_lora(), None when not disabled
        self._lora_raw = None     # ... the same factors by module: {module: [(adapter, A, B, alpha), ...]}; None when no adapter is loaded
        self._lora_w = None       # ... the factors in kernel layouts + the device table of scales, built on first use (_ensure_lora)
        self._lora_w_of = None
        self._lora_scale = 1.0    # ... set_lora_scale
        self._lora_id = 0         # ... identity of the loaded SET of adapters (graph key, cross-attention K / V cache key)
        self._lora_version = 0    # ... bumped by whatever changes the update (adapters, weights, scale): cached cross-attention K / V hold it
        self._freeu = None        # FreeU: (s1, s2, b1, b2) of enable_freeu, None when off
        self._freeu_dev = None    # ... the same four numbers as the float32 device table the kernel reads, built on first use

    # ------------------------------------------------------------------------------------------
    # structure
    # ------------------------------------------------------------------------------------------
    def _layout(self):
        """Yield the block structure shared by expected_keys / _prepare / forward."""
        c = self.config
        ch = list(c.block_out_channels)
        n = c.layers_per_block
        heads, depth = self._per_level(c.attention_head_dim), self._per_level(c.transformer_layers_per_block)
        downs, cout = [], ch[0]
        for i, t in enumerate(c.down_block_types):
            cin, cout = cout, ch[i]
            downs.append(dict(res=[(cin if j == 0 else cout, cout) for j in range(n)], attn=t.startswith("CrossAttn"),
                              down=i != len(ch) - 1, c=cout, heads=heads[i], depth=depth[i]))
        rev, rheads, rdepth = list(reversed(ch)), list(reversed(heads)), list(reversed(depth))
        ups, cout = [], rev[0]
        for i, t in enumerate(c.up_block_types):
            cprev, cout = cout, rev[i]
            cin = rev[min(i + 1, len(ch) - 1)]
            res = []
            for j in range(n + 1):
                skip = cin if j == n else cout
                rin = cprev if j == 0 else cout
                res.append((rin + skip, cout))
            ups.append(dict(res=res, attn=t.startswith("CrossAttn"), up=i != len(ch) - 1, c=cout, heads=rheads[i], depth=rdepth[i]))
        return downs, ups

    def _per_level(self, v):
        """An int or one value per resolution level (``attention_head_dim`` = heads, ``transformer_layers_per_block``)."""
        L = len(self.config.block_out_channels)
        v = list(v) if isinstance(v, (list, tuple)) else [v] * L
        if len(v) != L:
            raise ValueError(f"expected one value per level ({L}), got {v}")
        return v

    def expected_keys(self):
        c = self.config
        ch = list(c.block_out_channels)
        temb, cross = ch[0] * 4, c.cross_attention_dim
        keys = {}

        def conv(k, co, ci, ks):
            keys[k + ".weight"], keys[k + ".bias"] = (co, ci, ks, ks), (co,)

        def lin(k, co, ci, bias=True):
            keys[k + ".weight"] = (co, ci)
            if bias:
                keys[k + ".bias"] = (co,)

        def norm(k, n):
            keys[k + ".weight"], keys[k + ".bias"] = (n,), (n,)

        def resnet(k, ci, co):
            norm(k + ".norm1", ci); conv(k + ".conv1", co, ci, 3); lin(k + ".time_emb_proj", co, temb)
            norm(k + ".norm2", co); conv(k + ".conv2", co, co, 3)
            if ci != co:
                conv(k + ".conv_shortcut", co, ci, 1)

        def transformer(k, d, depth):
            norm(k + ".norm", d)
            if c.use_linear_projection:
                lin(k + ".proj_in", d, d); lin(k + ".proj_out", d, d)
            else:
                conv(k + ".proj_in", d, d, 1); conv(k + ".proj_out", d, d, 1)
            for n_ in range(depth):
                b = f"{k}.transformer_blocks.{n_}"
                for nm in ("norm1", "norm2", "norm3"):
                    norm(f"{b}.{nm}", d)
                for a, kd in (("attn1", d), ("attn2", cross)):
                    lin(f"{b}.{a}.to_q", d, d, False); lin(f"{b}.{a}.to_k", d, kd, False); lin(f"{b}.{a}.to_v", d, kd, False)
                    lin(f"{b}.{a}.to_out.0", d, d)
                lin(f"{b}.ff.net.0.proj", 8 * d, d); lin(f"{b}.ff.net.2", d, 4 * d)

        conv("conv_in", ch[0], c.in_channels, 3)
        lin("time_embedding.linear_1", temb, ch[0]); lin("time_embedding.linear_2", temb, temb)
        if c.time_cond_proj_dim is not None:  # guidance-embedded (LCM) UNets: diffusers TimestepEmbedding.cond_proj, no bias
            lin("time_embedding.cond_proj", ch[0], c.time_cond_proj_dim, False)
        if c.addition_embed_type == "text_time":
            lin("add_embedding.linear_1", temb, c.projection_class_embeddings_input_dim); lin("add_embedding.linear_2", temb, temb)
        downs, ups = self._layout()
        for i, blk in enumerate(downs):
            for j, (ci, co) in enumerate(blk["res"]):
                resnet(f"down_blocks.{i}.resnets.{j}", ci, co)
                if blk["attn"]:
                    transformer(f"down_blocks.{i}.attentions.{j}", co, blk["depth"])
            if blk["down"]:
                conv(f"down_blocks.{i}.downsamplers.0.conv", blk["c"], blk["c"], 3)
        resnet("mid_block.resnets.0", ch[-1], ch[-1]); transformer("mid_block.attentions.0", ch[-1], downs[-1]["depth"])
        resnet("mid_block.resnets.1", ch[-1], ch[-1])
        for i, blk in enumerate(ups):
            for j, (ci, co) in enumerate(blk["res"]):
                resnet(f"up_blocks.{i}.resnets.{j}", ci, co)
                if blk["attn"]:
                    transformer(f"up_blocks.{i}.attentions.{j}", co, blk["depth"])
            if blk["up"]:
                conv(f"up_blocks.{i}.upsamplers.0.conv", blk["c"], blk["c"], 3)
        norm("conv_norm_out", ch[0]); conv("conv_out", c.out_channels, ch[0], 3)
        return keys

    # ------------------------------------------------------------------------------------------
    # loading
    # ------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path, subfolder=None, torch_dtype=None, **config_overrides):
        """Read a diffusers-layout directory (``config.json`` + ``diffusion_pytorch_model.safetensors``).
        Extra kwargs override config entries, as scripts/inference/generate_hdr.py:138-142 does
        (``in_channels=8, **config``)."""
        d = os.path.join(path, subfolder) if subfolder else path
        cfg = cls.load_config(d)
        cfg.update(config_overrides)
        m = cls(**cfg)
        m.load_state_dict(read_state_dict(d))
        if torch_dtype is not None:
            m.to(torch_dtype)
        return m

    def save_pretrained(self, directory):
        import json
        from safetensors.torch import save_file

        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, "config.json"), "w") as f:
            json.dump({"_class_name": "UNet2DConditionModel", **{k: (list(v) if isinstance(v, tuple) else v) for k, v in self.config.items()}}, f, indent=2)
        save_file({k: v.contiguous() for k, v in self._raw.items()}, os.path.join(directory, "diffusion_pytorch_model.safetensors"))

    def replace_conv_in(self, in_channels=8):
        """The reference's ``_replace_unet_conv_in`` (scripts/inference/generate_hdr.py:75-94,
        scripts/stage2/train_gm_unet.py:658-677): widen ``conv_in`` to ``in_channels`` by repeating the weight along
        the input-channel axis and halving it; the bias is kept.  Returns self."""
        w, b = self._raw["conv_in.weight"], self._raw["conv_in.bias"]
        rep = in_channels // w.shape[1]
        if rep * w.shape[1] != in_channels:
            raise ValueError(f"in_channels={in_channels} is not a multiple of {w.shape[1]}")
        sd = dict(self._raw)
        sd["conv_in.weight"] = w.repeat(1, rep, 1, 1) * 0.5
        sd["conv_in.bias"] = b.clone()
        cfg = dict(self.config)
        cfg["in_channels"] = in_channels
        self._internal_dict = type(self._internal_dict)(cfg)
        return self.load_state_dict(sd)

    def init_random(self, seed=1234, device=None):
        """Deterministic synthetic weights (uniform +-1/sqrt(fan_in), unit norms) for benchmarks; no checkpoint
        exists offline.  ``device``: draw them with that device's generator instead of the host's (the
        multi-GPU bench: 8 ranks each drawing 1.8 G host randoms would be the longest phase of the run); the values then
        differ from the host draw but are the same on every rank."""
        g = torch.Generator(device or "cpu").manual_seed(seed)
        keys = self.expected_keys()
        sd = {}
        for k, shp in keys.items():
            if ".norm" in k or k.startswith("conv_norm_out") or k.endswith("norm.weight") or k.endswith("norm.bias"):
                sd[k] = torch.ones(shp) if k.endswith("weight") else torch.zeros(shp)
                continue
            wshape = keys[k.rsplit(".", 1)[0] + ".weight"]
            fan_in = 1
            for s_ in wshape[1:]:
                fan_in *= s_
            bound = fan_in ** -0.5
            sd[k] = (torch.rand(shp, generator=g, device=g.device) * 2 - 1) * bound
        return self.load_state_dict(sd)

    # ------------------------------------------------------------------------------------------
    # weight preparation
    # ------------------------------------------------------------------------------------------
    def _prepare_encoder(self, w):
        """conv_in, the time embedding, the down blocks and the mid block in kernel layouts, into ``w``: the half of the network a
        ControlNet shares with its UNet (components/controlnet.py prepares its copy with this very code).  Returns the builders and the
        running lists of the fused time-embedding projection, so that the caller can go on (the UNet: with its up blocks)."""
        c = self.config
        self._cin_pad = _pad_to(c.in_channels, self._kmul())
        w["conv_in"] = self._conv3("conv_in", self._cin_pad)
        w["te1"] = self._lin("time_embedding.linear_1")
        w["te2"] = self._lin("time_embedding.linear_2")
        if c.time_cond_proj_dim is not None:
            wc = self._raw["time_embedding.cond_proj.weight"]  # K = time_cond_proj_dim: zero-padded to the kernels' K multiple
            self._tcond_k = _pad_to(wc.shape[1], self._kmul())
            wp = torch.zeros(wc.shape[0], self._tcond_k)
            wp[:, : wc.shape[1]] = wc
            w["cond_proj"] = self._wt(wp)

        te_w, te_b = [], []
        self._transformers = []

        def resnet(k):
            r = dict(n1=self._norm(k + ".norm1"), c1=self._conv3(k + ".conv1"), n2=self._norm(k + ".norm2"), c2=self._conv3(k + ".conv2"))
            r["te_off"] = sum(t.shape[0] for t in te_w)  # column offset into the fused time-embedding projection
            te_w.append(self._raw[k + ".time_emb_proj.weight"])
            te_b.append(self._raw[k + ".time_emb_proj.bias"])
            if k + ".conv_shortcut.weight" in self._raw:
                r["sc"] = self._lin(k + ".conv_shortcut")
                # conv2 + shortcut as one launch (hip_ops.conv3x3_tail): [W2 | Wsc] packed once, the two biases summed in float32.  The
                # separate weights stay for the shapes whose plan has no K-tail loader and for GMD_FUSE_SHORTCUT=0.
                if ops.USE_SHORTCUT_FOLD and ops.is_half(self._dtype) and r["sc"][0].shape[1] % 64 == 0:
                    r["c2sc"] = ops.pack_shortcut(r["c2"][0], r["c2"][1], r["sc"][0], r["sc"][1])
            return r

        def transformer(k, heads, depth):
            """GroupNorm + proj_in / proj_out around ``depth`` BasicTransformerBlocks (1 for SD-1.5; 1 / 2 / 10 per level for SDXL)."""
            t = dict(norm=self._norm(k + ".norm"), pin=self._lin(k + ".proj_in"), pout=self._lin(k + ".proj_out"), heads=heads, blocks=[], key=k)
            for n_ in range(depth):
                b = f"{k}.transformer_blocks.{n_}"
                blk = dict(heads=heads)
                for nm in ("norm1", "norm2", "norm3"):
                    blk[nm] = self._norm(f"{b}.{nm}")
                q1, k1 = self._raw[f"{b}.attn1.to_q.weight"], self._raw[f"{b}.attn1.to_k.weight"]
                blk["v1"] = self._wa(self._raw[f"{b}.attn1.to_v.weight"])
                # q | k | v stacked: ONE launch writes Q|K row-major and V transposed (hip_ops.gemm_qkv_vt; 16-bit and float32 split modes)
                blk["qkv1"] = self._wt(torch.cat([q1, k1, self._raw[f"{b}.attn1.to_v.weight"]], 0))
                # fused [2C, C] projection of the fallback path.  16-bit modes: the first 2C rows of the stacked matrix (a contiguous
                # view, no third copy of q | k: ~62 MB per SD-1.5 UNet); the float32 split mode keeps its own copy, because a pre-split
                # weight carries ONE power-of-two scale for the whole matrix and q | k alone would get another
                blk["qk1"] = blk["qkv1"][: q1.shape[0] + k1.shape[0]] if ops.is_half(self._dtype) else self._wt(torch.cat([q1, k1], 0))
                blk["o1"] = self._lin(f"{b}.attn1.to_out.0")
                blk["q2"] = self._lin(f"{b}.attn2.to_q", False)[0]
                blk["k2"] = self._lin(f"{b}.attn2.to_k", False)[0]
                blk["v2"] = self._wa(self._raw[f"{b}.attn2.to_v.weight"])
                blk["o2"] = self._lin(f"{b}.attn2.to_out.0")
                if ops.is_half(self._dtype) or self._split_mode():
                    # fused GEGLU epilogue: interleave value / gate rows in groups of 16 so both land in the same MFMA lane
                    wf, bf = self._raw[f"{b}.ff.net.0.proj.weight"], self._raw[f"{b}.ff.net.0.proj.bias"]
                    half = wf.shape[0] // 2
                    wi = torch.stack([wf[:half].reshape(half // 16, 16, -1), wf[half:].reshape(half // 16, 16, -1)], 1).reshape(2 * half, -1)
                    bi = torch.stack([bf[:half].reshape(half // 16, 16), bf[half:].reshape(half // 16, 16)], 1).reshape(2 * half)
                    blk["ff1"] = (self._wt(wi), self._f32(bi))
                    blk["ff1_fused"] = True
                else:
                    blk["ff1"] = self._lin(f"{b}.ff.net.0.proj")
                    blk["ff1_fused"] = False
                blk["ff2"] = self._lin(f"{b}.ff.net.2")
                blk["key"] = b
                self._transformers.append(blk)  # every block has its own cross-attention K / V^T of the text tokens
                t["blocks"].append(blk)
            return t

        downs, _ = self._layout()
        w["down"] = []
        for i, blk in enumerate(downs):
            e = dict(res=[resnet(f"down_blocks.{i}.resnets.{j}") for j in range(len(blk["res"]))])
            if blk["attn"]:
                e["attn"] = [transformer(f"down_blocks.{i}.attentions.{j}", blk["heads"], blk["depth"]) for j in range(len(blk["res"]))]
            if blk["down"]:
                e["ds"] = self._conv3(f"down_blocks.{i}.downsamplers.0.conv")
            w["down"].append(e)
        w["mid"] = dict(r0=resnet("mid_block.resnets.0"), a=transformer("mid_block.attentions.0", downs[-1]["heads"], downs[-1]["depth"]),
                        r1=resnet("mid_block.resnets.1"))
        return resnet, transformer, te_w, te_b

    def _prepare(self):
        c = self.config
        w = {}
        resnet, transformer, te_w, te_b = self._prepare_encoder(w)
        _, ups = self._layout()
        if c.addition_embed_type == "text_time":
            wa = self._raw["add_embedding.linear_1.weight"]  # K = pooled text width + 6 sinusoids: zero-padded to the kernels' K multiple
            self._add_k = _pad_to(wa.shape[1], self._kmul())
            wp = torch.zeros(wa.shape[0], self._add_k)
            wp[:, : wa.shape[1]] = wa
            w["add1"] = (self._wt(wp), self._f32(self._raw["add_embedding.linear_1.bias"]))
            w["add2"] = self._lin("add_embedding.linear_2")
        w["up"] = []
        for i, blk in enumerate(ups):
            e = dict(res=[resnet(f"up_blocks.{i}.resnets.{j}") for j in range(len(blk["res"]))])
            if blk["attn"]:
                e["attn"] = [transformer(f"up_blocks.{i}.attentions.{j}", blk["heads"], blk["depth"]) for j in range(len(blk["res"]))]
            if blk["up"]:
                e["us"] = self._conv3(f"up_blocks.{i}.upsamplers.0.conv")
                # the four 2x2 phase weights of the exact-2x launch (hip_ops.conv3x3_up2), packed once; the nine-tap weight stays for
                # the sizes 2H - 1, the plans without a phase loader and GMD_UPSAMPLE_PHASES=0
                if ops.USE_UPSAMPLE_PHASES and ops.is_half(self._dtype) and e["us"][0].shape[1] % (9 * 64) == 0:
                    e["us4"] = ops.pack_upsample_phases(e["us"][0])[0]
            w["up"].append(e)
        w["norm_out"] = self._norm("conv_norm_out")
        w["conv_out"] = self._conv3("conv_out")
        # all ResnetBlock2D.time_emb_proj layers as ONE [sum(Cout), 1280] GEMM per forward
        w["te_all"] = (self._wt(torch.cat(te_w, 0)), self._f32(torch.cat(te_b, 0)))
        self._kv_cache = {}
        self._graphs = {}
        self._aug = {}
        self._tcond = {}
        self._t_dev = torch.zeros(1, dtype=torch.float32, device=self._device)
        return w

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    @staticmethod
    def _sa(*ws):
        """Store the activation that feeds these weights PRE-SPLIT (hip_ops: GMD_F32SA)?  Only when every consumer weight is itself
        pre-split, i.e. the float32 matrix-core mode; the producers then write [hi | lo] and the contractions skip their conversions."""
        return ops.USE_F32SA and all(getattr(w, "_split", False) for w in ws)

    def _resnet(self, r, x, B, H, W, temb, eps):
        G = self.config.norm_num_groups
        cs = self._wants_colstats(H, W)  # the GroupNorm that reads a conv output takes its statistics from the conv epilogue
        h = ops.groupnorm(x, B, G, r["n1"][0], r["n1"][1], eps, silu=True, split_out=self._sa(r["c1"][0]))
        # conv1 -> + time embedding -> norm2 -> SiLU: one GroupNorm launch over the split-K slabs on the 16x16 / 8x8 levels
        _, h = ops.conv3x3_groupnorm(h, r["c1"][0], B, H, W, G, r["n2"][0], r["n2"][1], eps, silu=True, bias=r["c1"][1],
                                     rowbias=(temb, r["te_off"]), colstats=cs, split_out=self._sa(r["c2"][0]))
        if "sc" in r:
            cin = x.shape[-1]
            if "c2sc" in r and ops.shortcut_fold_ok(self._dtype, B, H, W, h.shape[-1], cin, r["c2sc"][0].shape[0]):
                y, _, _ = ops.conv3x3_tail(h, x, r["c2sc"][0], B, H, W, bias=r["c2sc"][1], colstats=cs)
                return y
            ops.shortcut_launches += 1
            x = ops.gemm_nt(x.view(-1, cin), r["sc"][0], bias=r["sc"][1]).view(B, H * W, -1)
        y, _, _ = ops.conv3x3(h, r["c2"][0], B, H, W, bias=r["c2"][1], residual=x, colstats=cs)
        return y

    @staticmethod
    def _wants_colstats(H, W):
        """Levels whose GroupNorms take the two-launch split path (hip_ops.groupnorm): there the producer's epilogue
        statistics replace the statistics launch.  Smaller levels use the single-launch GroupNorm, which needs none."""
        return H * W >= 1024 and (H * W) % 64 == 0

    def _self_attention(self, t, n1, B, N, C):
        heads = t["heads"]
        d = C // heads
        scale = d ** -0.5
        lr = _lora_layer(self, t)  # None: the launches of a UNet without a LoRA adapter

        def adapted(qk2d, vt):
            # q | k: column ranges [0, C) / [C, 2C) of the stacked buffer; v: transposed, on whichever V^T this route produced
            if lr is not None:
                _lora_apply(self, lr, "attn1.to_q", n1, qk2d)
                _lora_apply(self, lr, "attn1.to_k", n1, qk2d, col=C)
                _lora_apply(self, lr, "attn1.to_v", n1, vt, tokens=N)
            return qk2d.view(B, N, 2 * C), vt

        if "qkv1" in t and (ops.is_half(self._dtype) or ops.split_attention_ok(self._dtype, d)):
            r = ops.gemm_qkv_vt(n1, t["qkv1"], 2 * C, N)
            if r is not None:
                qk, vt = adapted(r[0], r[1])
                return ops.attention(qk, qk, vt, heads, N, scale, k_col=C, split_out=self._sa(t["o1"][0]))
        qk = ops.gemm_nt(n1, t["qk1"])
        if ops.is_half(self._dtype) or ops.split_attention_ok(self._dtype, d):
            nv = n1.view(B, N, C)
            if ops.is_asplit(n1):  # a pre-split activation as the W operand of V^T = Wv n1^T: exactly the pre-split weight layout
                nv._split, nv._alpha = True, 1.0
            vt = ops.gemm_nt(t["v1"], nv, ldc=_pad_to(N, 8 if ops.is_half(self._dtype) else 4))  # V^T [B, C, N]
            qk, vt = adapted(qk, vt)
            return ops.attention(qk, qk, vt, heads, N, scale, k_col=C, split_out=self._sa(t["o1"][0]))
        npad = _pad_to(N, 4)
        if npad != N:
            vt = torch.zeros((B, C, npad), dtype=self._dtype, device=n1.device)
            ops.gemm_nt(t["v1"], n1.view(B, N, C), out=vt, ldc=npad)
        else:
            vt = ops.gemm_nt(t["v1"], n1.view(B, N, C), ldc=npad)
        qk, vt = adapted(qk, vt)
        return composed_attention(qk, 0, 2 * C, qk, C, 2 * C, vt, B, heads, d, N, N, scale, self._dtype)

    def _cross_kv(self, t, ehs):
        """K and V^T of the text tokens: constant over the whole denoising loop, so computed once per embedding tensor.
        The buffers are persistent per (layer, shape) and rewritten in place for new embeddings, so a captured HIP
        graph of the forward keeps reading valid addresses."""
        lr = _lora_layer(self, t)
        # with an adapter the cached K / V^T hold its update AT ITS SCALE: the key carries the adapter's identity and version
        key = (ehs.data_ptr(), ehs._version, tuple(ehs.shape), _lora_key(self))
        B, L, E = ehs.shape
        # one persistent buffer pair per (layer, batch, tokens): a graph captured for one batch size must keep finding ITS
        # buffers after the model has served another batch size in between
        slot = (t["key"], B, L, self._dtype)
        ent = self._kv_cache.get(slot)
        if ent is not None and ent["key"] == key:
            return ent["kc"], ent["vt"]
        if self._capturing:
            raise HipExtensionError("cross-attention K/V must be prepared (update_context) before graph capture")
        C = t["k2"].shape[0]
        lpad = _pad_to(L, 8 if ops.is_half(self._dtype) else 4)
        if ent is None:
            ent = dict(kc=torch.empty((B, L, C), dtype=self._dtype, device=ehs.device),
                       vt=torch.zeros((B, C, lpad), dtype=self._dtype, device=ehs.device))
            self._kv_cache[slot] = ent
        ops.gemm_nt(ehs.view(B * L, E), t["k2"], out=ent["kc"].view(B * L, C))
        ops.gemm_nt(t["v2"], ehs, out=ent["vt"], ldc=lpad)
        if lr is not None:  # a text-side LoRA: once per call on the text tokens, nothing per step
            _lora_apply(self, lr, "attn2.to_k", ehs.view(B * L, E), ent["kc"].view(B * L, C))
            _lora_apply(self, lr, "attn2.to_v", ehs.view(B * L, E), ent["vt"], tokens=L)
        ent["key"] = key
        ent["ehs"] = ehs  # holding `ehs` keeps its address from being recycled while the key is valid
        return ent["kc"], ent["vt"]

    @_in_own_f32_mode
    def update_context(self, ehs):
        """Prepare the cross-attention K / V^T of every transformer block for these text hidden states (eager,
        in place).  Called once per pipeline call; required before replaying a captured forward."""
        self._ensure()
        if getattr(self, "_lora_raw", None) is not None:
            self._ensure_lora()
        for t in self._transformers:
            self._cross_kv(t, ehs)

    # ------------------------------------------------------------------------------------------
    # IP-Adapter (image prompt): diffusers' load_ip_adapter / IPAdapterAttnProcessor / ImageProjection, restated
    # ------------------------------------------------------------------------------------------
    def _ip_layer_table(self):
        """[(k, transformer-block key, inner dim)] of an adapter's ``{k}.to_k_ip`` / ``{k}.to_v_ip`` weights: one odd k per ``attn2``, in
        diffusers' ``attn_processors`` order -- down blocks, then up blocks, then the mid block; the ``attn1`` processors hold the
        even numbers.  Host arithmetic on the config only."""
        downs, ups = self._layout()
        rows = []
        for name, blocks in (("down_blocks", downs), ("up_blocks", ups)):
            for i, blk in enumerate(blocks):
                if blk["attn"]:
                    rows += [(f"{name}.{i}.attentions.{j}.transformer_blocks.{n}", blk["c"]) for j in range(len(blk["res"])) for n in range(blk["depth"])]
        rows += [(f"mid_block.attentions.0.transformer_blocks.{n}", downs[-1]["c"]) for n in range(downs[-1]["depth"])]
        return [(2 * i + 1, key, c) for i, (key, c) in enumerate(rows)]

    def ip_adapter_layers(self):
        """[(k, transformer-block key)]: which block the weights stored under number k belong to (see _ip_layer_table)."""
        return [(k, key) for k, key, _ in self._ip_layer_table()]

    def ip_adapter_expected_keys(self, tokens, clip_dim):
        """({image_proj key: shape}, {ip_adapter key: shape}) of a plain IP-Adapter with ``tokens`` image tokens per picture."""
        cross = self.config.cross_attention_dim
        proj = {"proj.weight": (tokens * cross, clip_dim), "proj.bias": (tokens * cross,), "norm.weight": (cross,), "norm.bias": (cross,)}
        kv = {}
        for k, _, c in self._ip_layer_table():
            kv[f"{k}.to_k_ip.weight"] = (c, cross)
            kv[f"{k}.to_v_ip.weight"] = (c, cross)
        return proj, kv

    def load_ip_adapter(self, state_dict):
        """Install a plain IP-Adapter: ``state_dict`` = {"image_proj": {...}, "ip_adapter": {...}} as diffusers reads it.
        ``image_proj``: ``proj.weight`` [T*cross_dim, clip_dim], ``proj.bias``, ``norm.weight``, ``norm.bias`` (ImageProjection: linear,
        reshape to T tokens, LayerNorm eps 1e-5); ``ip_adapter``: ``{k}.to_k_ip.weight`` / ``{k}.to_v_ip.weight`` [inner_dim, cross_dim]
        for the odd k of ip_adapter_layers().  Host work only; the device copies are made at the first prepare_ip_context."""
        if self._ip_raw is not None:
            raise NotImplementedError("an IP-Adapter is already loaded: several adapters at once are not implemented "
                                      "(unload_ip_adapter() first)")
        if not isinstance(state_dict, dict) or "image_proj" not in state_dict or "ip_adapter" not in state_dict:
            raise ValueError("load_ip_adapter expects {'image_proj': {...}, 'ip_adapter': {...}}")
        proj, kv = state_dict["image_proj"], state_dict["ip_adapter"]
        for k in proj:
            if "perceiver_resampler" in k:
                raise NotImplementedError(f"IP-Adapter FaceID (image_proj key {k!r}: perceiver_resampler) is not implemented")
            if "latents" in k:
                raise NotImplementedError(f"IP-Adapter Plus (image_proj key {k!r}: the Resampler's latents) is not implemented")
            if k.startswith("proj.0.") or ".proj.0." in k:
                raise NotImplementedError(f"IP-Adapter Full-Face (image_proj key {k!r}: the MLP projection) is not implemented")
        for k in ("proj.weight", "proj.bias", "norm.weight", "norm.bias"):
            if k not in proj:
                raise KeyError(f"load_ip_adapter: image_proj.{k} is missing")
        cross = self.config.cross_attention_dim
        pw = proj["proj.weight"]
        if pw.dim() != 2 or pw.shape[0] % cross or pw.shape[0] == 0:
            raise ValueError(f"shape mismatch for image_proj.proj.weight: expected [T*{cross}, clip_dim], found {tuple(pw.shape)}")
        tokens, clip_dim = pw.shape[0] // cross, pw.shape[1]
        want_proj, want_kv = self.ip_adapter_expected_keys(tokens, clip_dim)
        missing = [k for k in want_kv if k not in kv]
        unexpected = [k for k in kv if k not in want_kv]
        if missing or unexpected:
            raise KeyError(f"load_ip_adapter: ip_adapter missing={missing[:5]} (+{max(len(missing) - 5, 0)}) "
                           f"unexpected={unexpected[:5]} (+{max(len(unexpected) - 5, 0)})")
        for part, want, got in (("image_proj", want_proj, proj), ("ip_adapter", want_kv, kv)):
            for k, shp in want.items():
                if tuple(got[k].shape) != tuple(shp):
                    raise ValueError(f"shape mismatch for {part}.{k}: expected {tuple(shp)}, found {tuple(got[k].shape)}")
        cpu = lambda t: t.detach().to("cpu", torch.float32)
        self._ip_raw = dict(tokens=tokens, clip_dim=clip_dim, proj={k: cpu(proj[k]) for k in want_proj}, kv={k: cpu(kv[k]) for k in want_kv})
        self._drop_ip_device_state()
        return self

    def unload_ip_adapter(self):
        """Back to the UNet without an image prompt: the launches, and so the outputs, of a model that never had one."""
        self._ip_raw = None
        self._ip_scale = 1.0
        self._drop_ip_device_state()
        return self

    def _drop_ip_device_state(self):
        self._ip_w = self._ip_w_of = self._ip_last = None
        self._ip_kv = {}
        # captured forwards that read the dropped buffers (key element ("ip", rows, Nip)); the others never touched them
        self._graphs = {k: g for k, g in self._graphs.items() if not any(isinstance(e, tuple) and e[:1] == ("ip",) for e in k)}

    @property
    def has_ip_adapter(self):
        return self._ip_raw is not None

    def set_ip_adapter_scale(self, scale):
        """One scale for every cross-attention layer (default 1.0), written into the float32 device array the kernels read -- outside
        any captured graph, so a captured forward serves every scale."""
        if isinstance(scale, (list, tuple, dict)):
            raise NotImplementedError("set_ip_adapter_scale: per-adapter lists and per-block dicts are not implemented (one float)")
        if self._ip_raw is None:
            raise ValueError("set_ip_adapter_scale: no IP-Adapter is loaded")
        if self._capturing:
            raise HipExtensionError("the IP-Adapter scale must be set outside graph capture")
        self._ip_scale = float(scale)
        if self._ip_w is not None and self._ip_w_of is self._w:
            self._ip_w["scales"].copy_(torch.full((self._ip_w["scales"].numel(),), self._ip_scale, dtype=torch.float32))

    def _ensure_ip(self):
        """The adapter's weights in kernel layouts, next to (and for) the prepared UNet weights."""
        self._ensure()
        if self._ip_raw is None:
            raise ValueError("this UNet has no IP-Adapter: call load_ip_adapter() first (image_embeds given)")
        if self._ip_w is not None and self._ip_w_of is self._w:
            return self._ip_w
        if self._capturing:
            raise HipExtensionError("the IP-Adapter must be prepared (prepare_ip_context) before graph capture")
        raw = self._ip_raw
        kpad = _pad_to(raw["clip_dim"], self._kmul())  # K = clip_dim: zero-padded to the kernels' K multiple
        wp = torch.zeros(raw["proj"]["proj.weight"].shape[0], kpad)
        wp[:, : raw["clip_dim"]] = raw["proj"]["proj.weight"]
        layers = self.ip_adapter_layers()
        w = dict(proj=(self._wt(wp), self._f32(raw["proj"]["proj.bias"])), kpad=kpad,
                 norm=(self._f32(raw["proj"]["norm.weight"]), self._f32(raw["proj"]["norm.bias"])), layers={},
                 scales=torch.full((len(layers),), self._ip_scale, dtype=torch.float32, device=self._device))
        for i, (k, blk) in enumerate(layers):
            w["layers"][blk] = dict(k=self._wt(raw["kv"][f"{k}.to_k_ip.weight"]), v=self._wa(raw["kv"][f"{k}.to_v_ip.weight"]), index=i)
        self._ip_kv = {}
        self._ip_w, self._ip_w_of = w, self._w
        return w

    @staticmethod
    def _single_adapter_embeds(image_embeds):
        if isinstance(image_embeds, (list, tuple)):
            if len(image_embeds) != 1:
                raise NotImplementedError(f"image_embeds holds {len(image_embeds)} tensors: several IP-Adapters at once are not implemented")
            image_embeds = image_embeds[0]
        if not torch.is_tensor(image_embeds) or image_embeds.dim() not in (2, 3):
            raise ValueError("image_embeds must be a tensor [rows, n_images, clip_dim] (or [rows, clip_dim])")
        return image_embeds if image_embeds.dim() == 3 else image_embeds.unsqueeze(1)

    def prepare_ip_context(self, image_embeds):
        """image_embeds [rows, n_images, clip_dim] (rows ordered like the text rows: [negative; positive] under guidance) -> the image
        prompt context ``forward_packed(ip=...)`` takes.  Runs ImageProjection (linear, T tokens per image, LayerNorm eps 1e-5) into
        the IP tokens [rows, n_images*T, cross_dim], then K_ip and V_ip^T of every transformer block, exactly as _cross_kv does for
        the text: persistent buffers per (layer, rows, Nip, dtype), rewritten in place, so a captured forward keeps reading valid
        addresses.  Eager HIP launches, once per pipeline call."""
        if self._ip_raw is None:
            raise ValueError("this UNet has no IP-Adapter: call load_ip_adapter() first (image_embeds given)")
        raw = self._ip_raw
        if not torch.is_tensor(image_embeds) or image_embeds.dim() != 3 or image_embeds.shape[2] != raw["clip_dim"]:
            raise ValueError(f"image_embeds must be [rows, n_images, {raw['clip_dim']}] "
                             f"(got {tuple(image_embeds.shape) if torch.is_tensor(image_embeds) else type(image_embeds).__name__})")
        rows, n_img, clip = image_embeds.shape
        T = raw["tokens"]
        nip = n_img * T
        if nip > ops.ATTN_IP_MAX_KEYS:
            raise ValueError(f"{n_img} images x {T} tokens = {nip} image keys: at most {ops.ATTN_IP_MAX_KEYS} (one key tile) are supported")
        if rows == 0 or n_img == 0:
            raise ValueError("image_embeds is empty")
        if not image_embeds.is_cuda:
            raise HipExtensionError("image_embeds must be on the HIP device")
        if self._capturing:
            raise HipExtensionError("the image prompt must be prepared (prepare_ip_context) before graph capture")
        return self._project_ip(image_embeds)

    @_in_own_f32_mode
    def _project_ip(self, image_embeds):
        """The device work of prepare_ip_context (its argument checks are host-only and come first)."""
        raw = self._ip_raw
        rows, n_img, clip = image_embeds.shape
        T = raw["tokens"]
        nip = n_img * T
        w = self._ensure_ip()
        # the same tensor again (the generic loop hands it over at every step): the buffers already hold its K_ip / V_ip^T
        key = (image_embeds.data_ptr(), image_embeds._version, tuple(image_embeds.shape), image_embeds.dtype)
        if self._ip_last is not None and self._ip_last[0] == key and self._ip_last[1].owner is w:
            return self._ip_last[1]
        cross = self.config.cross_attention_dim
        src = image_embeds.contiguous()
        if src.dtype != self._dtype:
            src = ops.cast(src if src.dtype in (torch.float32, torch.bfloat16, torch.float16) else src.float(), self._dtype)
        src = src.view(rows * n_img, clip)
        if w["kpad"] != clip:
            pad = torch.zeros((rows * n_img, w["kpad"]), dtype=self._dtype, device=self._device)
            pad[:, :clip].copy_(src)
            src = pad
        tok = ops.gemm_nt(src, w["proj"][0], bias=w["proj"][1]).view(rows * nip, cross)
        tok = ops.layernorm(tok, w["norm"][0], w["norm"][1], 1e-5).view(rows, nip, cross)
        lpad = _pad_to(nip, 8 if ops.is_half(self._dtype) else 4)
        for blk, lw in w["layers"].items():
            C = lw["k"].shape[0]
            slot = (blk, rows, nip, self._dtype)
            ent = self._ip_kv.get(slot)
            if ent is None:
                ent = self._ip_kv[slot] = dict(kc=torch.empty((rows, nip, C), dtype=self._dtype, device=self._device),
                                               vt=torch.zeros((rows, C, lpad), dtype=self._dtype, device=self._device))
            ops.gemm_nt(tok.view(rows * nip, cross), lw["k"], out=ent["kc"].view(rows * nip, C))
            ops.gemm_nt(lw["v"], tok, out=ent["vt"], ldc=lpad)
        ctx = _IPContext(rows, nip, tok, w)
        self._ip_last = (key, ctx, image_embeds)  # holding the tensor keeps its address from being recycled while the key is valid
        return ctx

    def _check_ip(self, ip, B):
        if not isinstance(ip, _IPContext) or ip.owner is not self._ip_w or self._ip_w_of is not self._w:
            raise HipExtensionError("ip: not a context of this UNet's current adapter (prepare_ip_context again after loading or moving)")
        if ip.rows != B:
            raise ValueError(f"the image prompt has {ip.rows} rows, the batch {B}")

    def _ip_kv_of(self, t, B, ip):
        ent = self._ip_kv.get((t["key"], B, ip.nip, self._dtype))
        if ent is None:
            raise HipExtensionError("IP-Adapter K/V must be prepared (prepare_ip_context) before the forward / graph capture")
        return ent["kc"], ent["vt"], self._ip_w["layers"][t["key"]]["index"]

    # ------------------------------------------------------------------------------------------
    # LoRA: adapters kept in factors and applied at run time (hip_ops.lora_update; several on one projection: lora_update_stacked);
    # components/lora.py reads the checkpoints and packs the stacks
    # ------------------------------------------------------------------------------------------
    def lora_module_names(self):
        """The model's own module names, the table kohya's flattened names are resolved against."""
        return [k[: -len(".weight")] for k in self.expected_keys() if k.endswith(".weight")]

    def load_lora(self, state_dict, ignore_unsupported=False, targets="attention", adapter_name=None):
        """Load a LoRA adapter (PEFT / diffusers / kohya keys: components/lora.py) for the attention projections of the transformer
        blocks; ``targets="transformer"`` also takes the feed-forward's ``ff.net.0.proj`` / ``ff.net.2`` and the transformers'
        ``proj_in`` / ``proj_out``.  Host work only: the factors go to the device, in the model's dtype and beside the prepared weights,
        at first use.  No weight buffer changes: every targeted projection is followed by one ``hip_ops.lora_update`` (``ff.net.0.proj``:
        by ``hip_ops.lora_geglu``, the update and the GEGLU in one launch; a block with a feed-forward target leaves ff_geglu_fused).

        May be called repeatedly: each call adds one adapter under ``adapter_name`` (default ``default_0``, ``default_1``, ... as in
        diffusers; a name already loaded is a ``ValueError``) with weight 1.0; ``targets`` / ``ignore_unsupported`` are per adapter.
        The SAME adapter a second time (equal factors on the same modules, under whatever name) is refused as already loaded -- it
        would silently double its effect, which ``set_adapters(name, 2.0)`` says in the open.  Both refusals, an unknown name and a
        state dict without factors raise ``lora.LoraAdapterError``, a ``ValueError`` that is also a ``NotImplementedError``.  A
        projection that two or more adapters target still takes ONE launch (``hip_ops.lora_update_stacked``: the factors side by side
        along the rank, a scale per rank column); each adapter's own rank stays <= 128, and ranks on one module that sum, after padding,
        to more than 256 raise ``NotImplementedError`` (naming the module, the ranks and the limit) and leave the model as it was."""
        from . import lora as _lora

        if self._capturing:
            raise HipExtensionError("a LoRA adapter must be loaded outside graph capture")
        if adapter_name is None:
            i = len(self._lora_adapters)
            while f"default_{i}" in self._lora_adapters:
                i += 1
            adapter_name = f"default_{i}"
        if not isinstance(adapter_name, str) or not adapter_name:
            raise ValueError(f"load_lora: adapter_name={adapter_name!r} must be a non-empty string")
        if adapter_name in self._lora_adapters:
            raise _lora.LoraAdapterError(f"load_lora: an adapter named {adapter_name!r} is already loaded (delete_adapters({adapter_name!r}) "
                                         "first)")
        parsed = _lora.parse_lora_state_dict(state_dict, self.lora_module_names(), ignore_unsupported=ignore_unsupported,
                                             targets=targets)
        if not parsed:
            raise _lora.LoraAdapterError("load_lora: the state dict holds no LoRA factors for this UNet's attention projections"
                                         + (", feed-forwards or proj_in / proj_out" if targets == "transformer" else ""))
        for other, loaded in self._lora_adapters.items():
            if _lora.same_adapter(parsed, loaded):
                raise _lora.LoraAdapterError(f"load_lora: this adapter is already loaded as {other!r} (the same factors on the same modules); "
                                             f"loading it twice is not implemented -- set_adapters({other!r}, 2.0) doubles its weight")
        shapes = self.expected_keys()
        for name, (a, b, _) in parsed.items():
            n, k = shapes[name + ".weight"][:2]
            if a.shape[1] != k or b.shape[0] != n:
                raise ValueError(f"load_lora: {name}: factors {tuple(b.shape)} x {tuple(a.shape)} do not fit the [{n}, {k}] projection")
        adapters = dict(self._lora_adapters)
        adapters[adapter_name] = parsed
        _lora.pack_adapters(adapters)  # the stacked ranks must fit: raises before anything of the model has changed
        if not self._lora_adapters:
            self._lora_scale = 1.0
        self._lora_weights[adapter_name] = 0.0 if self._lora_saved is not None else 1.0
        if self._lora_saved is not None:
            self._lora_saved[adapter_name] = 1.0
        self._set_lora_adapters(adapters)
        return self

    def _set_lora_adapters(self, adapters):
        """A new SET of adapters: layouts and launches change, so the device state and the ("lora",)-keyed graphs go."""
        self._lora_adapters = adapters
        self._lora_weights = {n: self._lora_weights[n] for n in adapters}
        if adapters:
            raw = {}
            for n, parsed in adapters.items():
                for m, (a, b, alpha) in parsed.items():
                    raw.setdefault(m, []).append((n, a, b, alpha))
            self._lora_raw = {m: raw[m] for m in sorted(raw)}
        else:
            self._lora_raw, self._lora_scale, self._lora_saved = None, 1.0, None
        _LORA_IDS[0] += 1
        self._lora_id = _LORA_IDS[0]
        self._drop_lora_device_state()

    def unload_lora(self):
        """Back to the UNet without an adapter (ALL adapters go): the launches, and so the outputs, of a model that never had one."""
        if self._capturing:
            raise HipExtensionError("LoRA adapters must be unloaded outside graph capture")
        self._lora_weights = {}
        self._set_lora_adapters({})
        return self

    def _drop_lora_device_state(self):
        self._lora_w = self._lora_w_of = None
        self._lora_version += 1  # cached cross-attention K / V^T were written with (or without) the dropped adapter
        self._graphs = {k: g for k, g in self._graphs.items() if not any(isinstance(e, tuple) and e[:1] == ("lora",) for e in k)}

    @property
    def has_lora(self):
        return self._lora_raw is not None

    def list_adapters(self):
        """The names of the loaded adapters, in load order."""
        return list(self._lora_adapters)

    def active_adapters(self):
        """The loaded adapters whose weight is not 0, in load order (none while ``disable_lora()`` holds)."""
        return [n for n in self._lora_adapters if self._lora_weights[n] != 0.0]

    def _known_adapters(self, what, names):
        from . import lora as _lora

        names = [names] if isinstance(names, str) else list(names)
        unknown = [n for n in names if n not in self._lora_adapters]
        if unknown:
            raise _lora.LoraAdapterError(f"{what}: no adapter named {unknown} is loaded (loaded: {self.list_adapters()})")
        if len(set(names)) != len(names):
            raise ValueError(f"{what}: a name is given twice in {names}")
        return names

    def set_adapters(self, names, weights=None):
        """diffusers' ``set_adapters``: ``names`` (one name or a list) become the active adapters with ``weights`` (one float per name,
        default 1.0); every other loaded adapter gets weight 0 -- its launches stay, its columns contribute nothing.  Unknown names are
        a ``ValueError``; per-block weight dicts (diffusers' ``{"down": ..., "mid": ..., "up": ...}``) are not implemented and refused
        by name.  Only the float32 device tables change (outside any graph capture): every captured graph is kept; the cross-attention
        K / V^T, cached WITH the update, are recomputed at the next ``update_context``."""
        names = self._known_adapters("set_adapters", names)
        if isinstance(weights, dict) or (isinstance(weights, (list, tuple)) and any(isinstance(w, dict) for w in weights)):
            raise NotImplementedError("set_adapters: per-block adapter weights (a dict per adapter) are not implemented: one float per adapter")
        if weights is None:
            weights = [1.0] * len(names)
        elif not isinstance(weights, (list, tuple)):
            weights = [weights] * len(names)
        if len(weights) != len(names):
            raise ValueError(f"set_adapters: {len(weights)} weights for {len(names)} adapters")
        weights = [1.0 if w is None else float(w) for w in weights]
        if not all(math.isfinite(w) for w in weights):
            raise ValueError(f"set_adapters: weights {weights} must be finite")
        new = {n: 0.0 for n in self._lora_adapters}
        new.update(zip(names, weights))
        self._lora_saved = None
        self._write_lora_tables(new, self._lora_scale)

    def delete_adapters(self, names):
        """Drop the named adapters (unknown names: ``ValueError``); the others keep their weights.  Layouts and launches change as at a
        load; a model brought back to ONE adapter launches and computes exactly what a model that only ever loaded that one does."""
        names = self._known_adapters("delete_adapters", names)
        if self._capturing:
            raise HipExtensionError("LoRA adapters must be deleted outside graph capture")
        if self._lora_saved is not None:
            self._lora_saved = {n: w for n, w in self._lora_saved.items() if n not in names}
        self._set_lora_adapters({n: p for n, p in self._lora_adapters.items() if n not in names})
        return self

    def disable_lora(self):
        """Every adapter weight to 0, remembered for ``enable_lora()``.  The LAUNCHES STAY -- each adds exactly 0 where its scale is 0
        -- so no graph is dropped and the result is that of the UNet without an adapter up to the roundings the feed-forward route of
        an adapted block differs by (an adapted block leaves ff_geglu_fused); ``unload_lora()`` gives the launches of a model that
        never had an adapter."""
        if self._lora_raw is None:
            raise ValueError("disable_lora: no LoRA adapter is loaded")
        if self._lora_saved is None:
            saved = dict(self._lora_weights)
            self._write_lora_tables({n: 0.0 for n in self._lora_adapters}, self._lora_scale)
            self._lora_saved = saved

    def enable_lora(self):
        """The weights ``disable_lora()`` remembered, back in the tables (nothing when it was not called)."""
        if self._lora_raw is None:
            raise ValueError("enable_lora: no LoRA adapter is loaded")
        if self._lora_saved is not None:
            saved, self._lora_saved = self._lora_saved, None
            self._write_lora_tables(saved, self._lora_scale)

    def set_lora_scale(self, scale):
        """The global LoRA scale (diffusers' ``cross_attention_kwargs={"scale": s}``; default 1.0), on top of the adapter weights: entry
        (module, adapter a) of the float32 device tables the kernels read is ``s * w_a * alpha_a / r_a``, rewritten outside any captured
        graph, so a captured forward serves every scale.  The cross-attention K / V^T are cached per prompt WITH the update, so they are
        recomputed at the next ``update_context``."""
        if self._lora_raw is None:
            raise ValueError("set_lora_scale: no LoRA adapter is loaded")
        self._write_lora_tables(self._lora_weights, float(scale))

    def _write_lora_tables(self, weights, scale):
        if self._capturing:
            raise HipExtensionError("the LoRA scale and adapter weights must be set outside graph capture")
        if scale == self._lora_scale and weights == self._lora_weights:
            return
        self._lora_weights, self._lora_scale = dict(weights), scale
        self._lora_version += 1
        if self._lora_w is not None and self._lora_w_of is self._w:
            from . import lora as _lora

            scalars, columns = _lora.scale_tables(self._lora_adapters, self._lora_w["packing"], self._lora_weights, self._lora_scale)
            self._lora_w["scales"].copy_(scalars)
            self._lora_w["colscales"].copy_(columns)

    # ------------------------------------------------------------------------------------------
    # FreeU: diffusers' UNet2DConditionModel.enable_freeu / disable_freeu (hip_ops.concat_channels_freeu in up blocks 0 and 1)
    # ------------------------------------------------------------------------------------------
    def enable_freeu(self, s1, s2, b1, b2, **unsupported):
        """FreeU ("Free Lunch in Diffusion U-Net"), as diffusers' ``enable_freeu``: in front of EVERY resnet of up blocks 0 and 1 the
        first half of the backbone channels is scaled by ``b1`` / ``b2`` and the skip goes through the Fourier filter that scales its
        lowest frequencies (threshold 1) by ``s1`` / ``s2``.  The skip concat of those six sites becomes ONE launch of
        ``hip_ops.concat_channels_freeu``; nothing else changes, no weight is touched, no extra UNet evaluation.

        All four values must be finite and > 0 (``ValueError`` naming the argument otherwise).  diffusers silently DISABLES FreeU when
        one of them is 0 (its up blocks test the attributes for truth); here that is refused -- call ``disable_freeu()``.

        The numbers live in one float32 device table the kernel reads: new numbers on an already-enabled model rewrite the table
        (outside any graph capture) and keep every captured graph.  Enabling changes the launches, so captured forwards of the enabled
        model are kept under a key with ("freeu",).  Not built: a filter threshold other than 1 (diffusers never passes another), the
        FreeU authors' "v2" backbone map, per-block settings, FreeU on the VAE or a ControlNet."""
        if unsupported:
            raise NotImplementedError(f"enable_freeu: unsupported arguments {sorted(unsupported)}: only diffusers' (s1, s2, b1, b2) is "
                                      "implemented -- no filter threshold other than 1, no 'v2' backbone map, no per-block settings")
        vals = []
        for name, v in (("s1", s1), ("s2", s2), ("b1", b1), ("b2", b2)):
            if isinstance(v, (list, tuple, dict)) or torch.is_tensor(v) and v.numel() != 1:
                raise NotImplementedError(f"enable_freeu: {name} must be one number (per-block settings are not implemented)")
            v = float(v)
            if not math.isfinite(v) or v <= 0.0:
                raise ValueError(f"enable_freeu: {name}={v!r} must be finite and > 0 (diffusers treats 0 as 'FreeU off': call disable_freeu())")
            vals.append(v)
        if self._capturing:
            raise HipExtensionError("the FreeU setting must be changed outside graph capture")
        self._freeu = tuple(vals)
        if self._freeu_dev is not None:
            self._freeu_dev.copy_(torch.tensor(self._freeu, dtype=torch.float32))
        return self

    def disable_freeu(self):
        """Back to the UNet without FreeU: the launches, and so the outputs, of a model that never had it."""
        if self._capturing:
            raise HipExtensionError("the FreeU setting must be changed outside graph capture")
        self._freeu = None
        self._graphs = {k: g for k, g in self._graphs.items() if ("freeu",) not in k}
        return self

    @property
    def freeu(self):
        """(s1, s2, b1, b2) of ``enable_freeu``, or None."""
        return self._freeu

    def _freeu_table(self):
        """The float32 device table [s1, s2, b1, b2] (hip_ops.FREEU_PARAMS entries) the kernel reads, on this model's device."""
        if self._freeu_dev is None or self._freeu_dev.device != self._t_dev.device:
            if self._capturing:
                raise HipExtensionError("the FreeU table must exist before graph capture")
            self._freeu_dev = torch.tensor(self._freeu, dtype=torch.float32).to(self._t_dev.device)
            assert self._freeu_dev.numel() == ops.FREEU_PARAMS
        return self._freeu_dev

    def _ensure_lora(self):
        """The adapters' factors in kernel layouts, next to (and for) the prepared UNet weights: the rank zero-padded to the multiple
        the contractions of this dtype mode need, ``a`` a W operand (pre-split where the weights are), ``b`` a W operand for the plain
        outputs and an A operand for the V^T outputs (as the model's own to_v weights).  A module one adapter targets: (a, b, slot in
        the table of scalar scales).  A module several target: a ``_LoraStack`` -- the stacked factors and the row of column scales
        in the 16-bit types, the adapters one by one where the sequential route runs (float32, GMD_LORA_STACK_FUSED=0)."""
        self._ensure()
        if self._lora_w is not None and self._lora_w_of is self._w:
            return self._lora_w
        if self._capturing:
            raise HipExtensionError("the LoRA adapter must be prepared (update_context) before graph capture")
        from . import lora as _lora

        mult = ops.lora_rank_multiple(self._dtype, split=self._split_mode())
        stack_fused = ops.is_half(self._dtype) and ops.USE_LORA_STACK_FUSED
        packing = _lora.pack_adapters(self._lora_adapters)
        layers = {}
        for name, mp in packing.modules.items():
            interleave = False
            if name.endswith(_lora.FF_SUFFIXES):
                blk, proj = name.split(".ff.net.", 1)
                proj = "ff.net." + proj
                # the row order of the block's ff1 weight (_prepare_encoder): y's columns arrive in it
                interleave = proj == "ff.net.0.proj" and (ops.is_half(self._dtype) or self._split_mode())
            elif name.endswith(_lora.PROJ_SUFFIXES):
                blk, proj = name.rsplit(".", 1)  # the Transformer2DModel itself
            else:
                blk, proj = name.rsplit(".attn", 1)
                proj = "attn" + proj

            def device_pair(ap, bp):
                if interleave:
                    bp = ops.geglu_interleave(bp)
                return self._wt(ap), self._wa(bp) if proj.endswith("to_v") else self._wt(bp)

            def padded_pair(n):
                a, b, _ = self._lora_adapters[n][name]
                r = a.shape[0]
                rp = _pad_to(r, mult)
                ap, bp = torch.zeros(rp, a.shape[1]), torch.zeros(b.shape[0], rp)
                ap[:r], bp[:, :r] = a, b
                return device_pair(ap, bp)

            if not mp.stacked:
                ent = padded_pair(mp.adapters[0]) + (mp.slots[0],)
            elif stack_fused:
                ent = _LoraStack(*device_pair(*_lora.stack_factors(self._lora_adapters, name, mp)), mp.row, None)
            else:
                ent = _LoraStack(None, None, mp.row, [padded_pair(n) + (i,) for n, i in zip(mp.adapters, mp.slots)])
            layers.setdefault(blk, {})[proj] = ent
        scalars, columns = _lora.scale_tables(self._lora_adapters, packing, self._lora_weights, self._lora_scale)
        w = dict(layers=layers, packing=packing, scales=scalars.to(self._device), colscales=columns.to(self._device))
        self._lora_w, self._lora_w_of = w, self._w
        return w

    @staticmethod
    def _dup_batch(t):
        """[B, ...] -> [2B, ...]: both halves equal to ``t`` (gmd_dup_batch: one read, two writes)."""
        out = ops.dup_batch(t.contiguous())
        st = getattr(t, "_colstats", None)
        if st is not None and not isinstance(st, list):  # producer statistics are per 64-row block, sample-major: duplicate alike
            out._colstats = (torch.cat([st[0], st[0]], 0), st[1])
        return out

    def _transformer(self, t, x, B, H, W, ehs, cfg_dup=False, ip=None):
        """``cfg_dup``: x holds the B UNIQUE samples of a classifier-free-guidance pair whose two halves differ only in the
        text conditioning; everything up to the first cross-attention query is computed once, then duplicated (returns 2B rows)."""
        C = x.shape[-1]
        N = H * W
        lt = _lora_layer(self, t)  # the adapter's proj_in / proj_out factors of this transformer, or None
        g = ops.groupnorm(x, B, self.config.norm_num_groups, t["norm"][0], t["norm"][1], 1e-6, silu=False, split_out=self._sa(t["pin"][0]))
        h = ops.gemm_nt(g.view(B * N, C), t["pin"][0], bias=t["pin"][1], a_split=ops.is_asplit(g))  # conv1x1 and nn.Linear proj_in are the same GEMM on tokens
        if lt is not None:  # (under cfg_dup: on the B unique rows)
            _lora_apply(self, lt, "proj_in", g.view(B * N, C), h, x_split=ops.is_asplit(g))
        for blk in t["blocks"]:
            h, x, B = self._transformer_block(blk, h, x, B, N, C, ehs, cfg_dup, ip)
            cfg_dup = False  # the first cross-attention has duplicated the batch
        # an adapted proj_out: the epilogue's column statistics would describe the tensor BEFORE the update, so none are produced and
        # the next GroupNorm (or concat) computes its own (hip_ops._usable_colstats: a tensor without ._colstats)
        pout_lora = lt is not None and "proj_out" in lt
        y = ops.gemm_nt(h, t["pout"][0], bias=t["pout"][1], residual=x.view(B * N, C), colstats=self._wants_colstats(H, W) and not pout_lora)
        if pout_lora:  # after the bias + residual epilogue: the update commutes with both
            _lora_apply(self, lt, "proj_out", h, y, x_split=ops.is_asplit(h))
        return ops.carry_colstats(y.view(B, N, C), y)

    def _transformer_block(self, t, h, x, B, N, C, ehs, cfg_dup, ip=None):
        """One BasicTransformerBlock on tokens ``h`` [B*N, C]; returns (h, x, B) -- x / B change when ``cfg_dup`` duplicates.
        ``ip``: None (the launches of a UNet without an adapter), or the image-prompt context of prepare_ip_context: the cross-attention
        becomes the decoupled one, text branch + ip_scale * image branch."""
        heads = t["heads"]
        d = C // heads
        # self-attention
        # (the V^T product takes n1 as its W operand: pre-split only where the matrix-core attention path is taken)
        n1 = ops.layernorm(h, *t["norm1"], split_out=self._sa(t["qk1"]) and ops.split_attention_ok(self._dtype, d))
        lr = _lora_layer(self, t)  # None: the launches of a UNet without a LoRA adapter
        o = self._self_attention(t, n1, B, N, C)
        h = ops.gemm_nt(o.view(B * N, C), t["o1"][0], bias=t["o1"][1], residual=h, a_split=ops.is_asplit(o))
        if lr is not None:  # after the bias + residual epilogue: the update commutes with both
            _lora_apply(self, lr, "attn1.to_out.0", o.view(B * N, C), h, x_split=ops.is_asplit(o))
        # cross-attention over the text tokens
        n2 = ops.layernorm(h, *t["norm2"], split_out=self._sa(t["q2"]))
        q = ops.gemm_nt(n2, t["q2"])
        if lr is not None:  # (under cfg_dup: on the B unique rows, before the duplication)
            _lora_apply(self, lr, "attn2.to_q", n2, q)
        q = q.view(B, N, C)
        if cfg_dup:  # first use of the text conditioning: from here on the two halves differ
            q, h, x = self._dup_batch(q), self._dup_batch(h.view(B, N, C)).view(2 * B * N, C), self._dup_batch(x)
            B *= 2
        kc, vtc = self._cross_kv(t, ehs)
        L = ehs.shape[1]
        if ip is not None:
            kip, vtip, idx = self._ip_kv_of(t, B, ip)
            if ops.is_half(self._dtype) or ops.split_attention_ok(self._dtype, d):
                # 16-bit: one launch (gmd_attention_ip); float32 on the matrix cores: two launches and the scaled add, plain float32 out
                o = ops.attention_ip(q, kc, vtc, kip, vtip, heads, L, ip.nip, d ** -0.5, self._ip_w["scales"], idx)
            else:
                o = composed_attention(q, 0, C, kc, 0, C, vtc, B, heads, d, N, L, d ** -0.5, self._dtype)
                oi = composed_attention(q, 0, C, kip, 0, C, vtip, B, heads, d, N, ip.nip, d ** -0.5, self._dtype)
                o = ops.scaled_add(o, oi, self._ip_w["scales"], idx, out=o)
        elif ops.is_half(self._dtype) or ops.split_attention_ok(self._dtype, d):
            o = ops.attention(q, kc, vtc, heads, L, d ** -0.5, split_out=self._sa(t["o2"][0]))
        else:
            o = composed_attention(q, 0, C, kc, 0, C, vtc, B, heads, d, N, L, d ** -0.5, self._dtype)
        h = ops.gemm_nt(o.view(B * N, C), t["o2"][0], bias=t["o2"][1], residual=h, a_split=ops.is_asplit(o))
        if lr is not None:
            _lora_apply(self, lr, "attn2.to_out.0", o.view(B * N, C), h, x_split=ops.is_asplit(o))
        # GEGLU feed-forward
        n3 = ops.layernorm(h, *t["norm3"], split_out=self._sa(t["ff1"][0]))
        if lr is not None and ("ff.net.0.proj" in lr or "ff.net.2" in lr):  # an adapted feed-forward: two GEMMs, no ff_geglu_fused
            return self._feed_forward_lora(t, lr, n3, h), x, B
        if t["ff1_fused"] and ops.ff_fused_ok(n3, C):  # the whole feed-forward in one launch: [tokens, 4C] never reaches HBM
            h = ops.ff_geglu_fused(n3, t["ff1"][0], t["ff1"][1], t["ff2"][0], t["ff2"][1], h)
        else:
            if t["ff1_fused"]:  # h * gelu(g) formed in the GEMM epilogue (float32 matrix-core mode: stored pre-split for ff2)
                f = ops.gemm_nt(n3, t["ff1"][0], bias=t["ff1"][1], act=ops.ACT_GEGLU, split_out=self._sa(t["ff2"][0]))
            else:
                f = ops.geglu(ops.gemm_nt(n3, t["ff1"][0], bias=t["ff1"][1]))
            h = ops.gemm_nt(f, t["ff2"][0], bias=t["ff2"][1], residual=h)
        return h, x, B

    def _feed_forward_lora(self, t, lr, n3, h):
        """The feed-forward of a block whose ``ff.net.0.proj`` and / or ``ff.net.2`` is adapted.  The first update has to land in
        front of the gate, so the first GEMM stores the plain pre-activation [tokens, 8C] and ``hip_ops.lora_geglu`` forms
        (value + update) * gelu(gate + update) from it in one launch; the second update commutes with ff2's bias and residual, as at
        to_out.0."""
        scales = self._lora_w["scales"]
        e1 = lr.get("ff.net.0.proj")
        if e1 is not None:
            y = ops.gemm_nt(n3, t["ff1"][0], bias=t["ff1"][1])
            if not t["ff1_fused"]:  # float32 exact: [value half | gate half]
                _lora_apply(self, lr, "ff.net.0.proj", n3, y)
                f = ops.geglu(y)
            elif isinstance(e1, _LoraStack):  # several adapters: still one launch for the update and the GEGLU
                f = ops.lora_geglu_stacked(n3, e1.a, e1.b, y, self._lora_w["colscales"], e1.row, x_split=ops.is_asplit(n3),
                                           parts=e1.seq(scales))
            else:  # interleaved ff1 rows (16-bit, float32 split): e1's b rows are permuted alike (_ensure_lora)
                f = ops.lora_geglu(n3, e1[0], e1[1], y, scales, e1[2], x_split=ops.is_asplit(n3))
        elif t["ff1_fused"]:
            f = ops.gemm_nt(n3, t["ff1"][0], bias=t["ff1"][1], act=ops.ACT_GEGLU, split_out=self._sa(t["ff2"][0]))
        else:
            f = ops.geglu(ops.gemm_nt(n3, t["ff1"][0], bias=t["ff1"][1]))
        h = ops.gemm_nt(f, t["ff2"][0], bias=t["ff2"][1], residual=h)
        _lora_apply(self, lr, "ff.net.2", f, h, x_split=ops.is_asplit(f))
        return h

    def set_timestep(self, timestep):
        """Write the timestep into the device scalar read by the embedding kernel (kept outside any
        captured graph so the same graph can be replayed for every step)."""
        self._ensure()
        t = float(timestep)
        self._t_dev.copy_(torch.tensor([t], dtype=torch.float32), non_blocking=False)

    def set_timestep_from(self, ts_dev, i):
        """Device-to-device variant: copy element ``i`` of a float32 device vector of timesteps (no host round trip,
        so the host can run ahead of the GPU)."""
        self._ensure()
        self._t_dev.copy_(ts_dev[i:i + 1], non_blocking=True)
        if getattr(self, "_stamp_buf", None) is not None:  # measurement hook: this iteration's row of the stamp table
            self._stamp_row.fill_(i)

    def supports_cfg_shared(self):
        """True when the first down block has a transformer (SD-1.5): the prefix shared by a CFG pair ends at its
        cross-attention."""
        c = self.config  # (a per-row conditioning of the time embedding may differ between the two halves: no shared prefix then)
        return c.down_block_types[0].startswith("CrossAttn") and c.addition_embed_type is None and c.time_cond_proj_dim is None

    @_in_own_f32_mode
    def set_added_cond(self, added_cond_kwargs, B):
        """SDXL micro-conditioning (diffusers ``get_aug_embed`` for addition_embed_type "text_time"): sinusoid of every scalar of
        ``time_ids`` [B, 6] concatenated behind the pooled text embedding ``text_embeds`` [B, P], through add_embedding.linear_1 ->
        SiLU -> linear_2; the result is ADDED to the time embedding in every forward.  Constant over the denoising loop: computed
        once per call here (eager, HIP kernels) into a persistent [B, temb] buffer that captured graphs keep reading."""
        self._ensure()
        c = self.config
        if c.addition_embed_type != "text_time":
            if added_cond_kwargs:
                raise NotImplementedError("this UNet has no addition embedding (added_cond_kwargs given)")
            return None
        if not added_cond_kwargs or "text_embeds" not in added_cond_kwargs or "time_ids" not in added_cond_kwargs:
            raise ValueError("this UNet needs added_cond_kwargs = {'text_embeds': [B, P], 'time_ids': [B, 6]} (addition_embed_type 'text_time')")
        te, ids = added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"]
        if te.shape[0] != B or ids.shape[0] != B or not te.is_cuda:
            raise ValueError(f"added_cond_kwargs must hold {B} device rows (got {tuple(te.shape)}, {tuple(ids.shape)})")
        d = c.addition_time_embed_dim
        P = te.shape[1]
        if P + ids.shape[1] * d != c.projection_class_embeddings_input_dim:
            raise ValueError("text_embeds / time_ids widths do not match projection_class_embeddings_input_dim")
        key = (te.data_ptr(), te._version, ids.data_ptr(), ids._version, B)
        ent = self._aug.get(B)
        if ent is not None and ent["key"] == key:
            return ent["aug"]
        if self._capturing:
            raise HipExtensionError("the added conditioning must be prepared (set_added_cond) before graph capture")
        cat = torch.zeros((B, self._add_k), dtype=self._dtype, device=self._device)
        tex = te.contiguous()
        if tex.dtype != self._dtype:
            tex = ops.cast(tex if tex.dtype in (torch.float32, torch.bfloat16, torch.float16) else tex.float(), self._dtype)
        cat[:, :P].copy_(tex)
        flat = ids.to(self._device, torch.float32).contiguous().view(-1)  # (a [B, 6] table of image sizes / crops given by the caller)
        for i in range(flat.numel()):  # one [1, d] sinusoid per scalar: the timestep-embedding kernel, reading the scalar on the device
            b, j = divmod(i, ids.shape[1])
            cat[b, P + j * d:P + (j + 1) * d].copy_(ops.timestep_embedding(flat[i:i + 1], 1, d, self._dtype, c.flip_sin_to_cos, c.freq_shift)[0])
        w = self._w
        a1 = ops.gemm_nt(cat, w["add1"][0], bias=w["add1"][1], act=ops.ACT_SILU)
        aug = ops.gemm_nt(a1, w["add2"][0], bias=w["add2"][1])
        if ent is None:
            ent = self._aug[B] = dict(aug=aug)
        else:
            ent["aug"].copy_(aug)  # in place: a captured graph keeps reading this buffer
        ent["key"] = key
        ent["src"] = (te, ids)  # keep the sources alive while the key is valid
        return ent["aug"]

    def _tcond_entry(self, B):
        """The persistent [B, ch0] buffer of ``cond_proj(timestep_cond)`` for batch ``B``; created as zeros (diffusers'
        ``timestep_cond=None``) on first use, never inside a graph capture."""
        ent = self._tcond.get(B)
        if ent is None:
            if self._capturing:
                raise HipExtensionError("the timestep conditioning must be prepared (set_timestep_cond) before graph capture")
            buf = torch.zeros((B, self.config.block_out_channels[0]), dtype=self._dtype, device=self._device)
            ent = self._tcond[B] = dict(buf=buf, key=None, src=None)
        return ent

    @_in_own_f32_mode
    def set_timestep_cond(self, cond, B):
        """Guidance-scale conditioning of a guidance-embedded (LCM) UNet (diffusers ``TimestepEmbedding.cond_proj``, config
        ``time_cond_proj_dim``): ``cond`` [B, time_cond_proj_dim] (the pipelines' ``get_guidance_scale_embedding``) goes through the
        bias-free projection once (eager, HIP GEMM) into a persistent [B, block_out_channels[0]] buffer in the UNet dtype, which
        every forward adds to the sinusoidal embedding in front of ``time_embedding.linear_1``.  None zeroes the buffer (diffusers'
        ``timestep_cond=None``).  Constant over the denoising loop; a captured graph keeps reading the buffer, rewritten in place
        here, so one capture serves every guidance scale."""
        self._ensure()
        d = self.config.time_cond_proj_dim
        if d is None:
            if cond is not None:
                raise ValueError("this UNet has no time_embedding.cond_proj (config time_cond_proj_dim is None): timestep_cond given")
            return None
        if cond is None:
            ent = self._tcond_entry(B)
            if ent["key"] is not None:
                if self._capturing:
                    raise HipExtensionError("the timestep conditioning must be prepared (set_timestep_cond) before graph capture")
                ent["buf"].zero_()
                ent["key"] = ent["src"] = None
            return ent["buf"]
        if cond.dim() != 2 or tuple(cond.shape) != (B, d) or not cond.is_cuda:
            raise ValueError(f"timestep_cond must be a device tensor of shape [{B}, {d}] (time_cond_proj_dim); got {tuple(cond.shape)}"
                             f" on {cond.device}")
        key = (cond.data_ptr(), cond._version, B)
        ent = self._tcond.get(B)
        if ent is not None and ent["key"] == key:
            return ent["buf"]
        if self._capturing:
            raise HipExtensionError("the timestep conditioning must be prepared (set_timestep_cond) before graph capture")
        ent = self._tcond_entry(B)
        src = cond.contiguous()
        if src.dtype != self._dtype:
            src = ops.cast(src if src.dtype in (torch.float32, torch.bfloat16, torch.float16) else src.float(), self._dtype)
        if self._tcond_k != d:
            pad = torch.zeros((B, self._tcond_k), dtype=self._dtype, device=self._device)
            pad[:, :d].copy_(src)
            src = pad
        ent["buf"].copy_(ops.gemm_nt(src, self._w["cond_proj"]))  # in place: a captured graph keeps reading this buffer
        ent["key"] = key
        ent["src"] = cond  # keep the source alive while the key is valid
        return ent["buf"]

    def _time_embedding(self, w, B):
        """The fused time-embedding projection of this forward: float32 [B, sum(Cout)] (every ResnetBlock2D's ``time_emb_proj`` of
        ``silu(time_embedding(t))`` in one GEMM), from the timestep in ``_t_dev``."""
        c = self.config
        if c.time_cond_proj_dim is None:
            te = ops.timestep_embedding(self._t_dev, B, c.block_out_channels[0], self._dtype, c.flip_sin_to_cos, c.freq_shift)
        else:  # t_emb.to(dtype) + cond_proj(timestep_cond) in ONE launch, as the plain embedding; zeros until set_timestep_cond
            te = ops.timestep_embedding_add(self._t_dev, self._tcond_entry(B)["buf"], B, c.block_out_channels[0], self._dtype,
                                            c.flip_sin_to_cos, c.freq_shift)
        te = ops.gemm_nt(te, w["te1"][0], bias=w["te1"][1], act=ops.ACT_SILU)
        aug = None
        if c.addition_embed_type == "text_time":  # emb = time_embedding(t) + add_embedding(...): the sum goes through the SiLU below
            ent = self._aug.get(B)
            if ent is None:
                raise HipExtensionError("this UNet needs its added conditioning first: set_added_cond(added_cond_kwargs, batch)")
            aug = ent["aug"]
        temb = ops.gemm_nt(te, w["te2"][0], bias=w["te2"][1], residual=aug, act=ops.ACT_SILU)  # = silu(temb): the only use of temb
        return ops.gemm_nt(temb, w["te_all"][0], bias=w["te_all"][1], out_dtype=torch.float32)  # [B, sum(Cout)] f32

    def _down_mid(self, w, x, B, Bc, H, W, temb, ehs, mark, cond=None, ip=None):
        """conv_in, the down blocks and the mid block on the packed input: the walk a ControlNet shares with its UNet.  ``Bc``: rows
        carried at the start (B / 2 under the CFG shared prefix); ``cond``: a tensor added to conv_in's output in its epilogue (the
        ControlNet's conditioning embedding; None for the UNet: the plain launch).  Returns (x, skips, H, W) with
        ``skips`` = [(tensor, h, w)] in the order diffusers collects ``down_block_res_samples``."""
        eps = self.config.norm_eps
        x, _, _ = ops.conv3x3(x, w["conv_in"][0], Bc, H, W, bias=w["conv_in"][1], residual=cond, colstats=self._wants_colstats(H, W))
        skips = [(x, H, W)]
        for blk in w["down"]:
            for j, r in enumerate(blk["res"]):
                x = self._resnet(r, x, Bc, H, W, temb[:Bc], eps)  # (both halves share the timestep: temb rows are identical)
                if "attn" in blk:
                    dup = Bc != B
                    x = self._transformer(blk["attn"][j], x, Bc, H, W, ehs, cfg_dup=dup, ip=ip)
                    if dup:
                        skips = [(self._dup_batch(s_), h_, w_) for s_, h_, w_ in skips]
                        Bc = B
                skips.append((x, H, W))
            if "ds" in blk:
                x, H, W = ops.conv3x3(x, blk["ds"][0], B, H, W, bias=blk["ds"][1], stride=2,
                                      colstats=self._wants_colstats((H + 1) // 2, (W + 1) // 2))  # stride 2, padding 1: ceil
                skips.append((x, H, W))
            mark()  # end of a down block
        x = self._resnet(w["mid"]["r0"], x, B, H, W, temb, eps)
        x = self._transformer(w["mid"]["a"], x, B, H, W, ehs, ip=ip)
        x = self._resnet(w["mid"]["r1"], x, B, H, W, temb, eps)
        mark()  # end of the mid block
        return x, skips, H, W

    @_in_own_f32_mode
    def forward_packed(self, x, B, H, W, encoder_hidden_states, cfg_shared=False, control=None, ip=None):
        """x: packed channels-last input [B, H*W, cin_pad]; the timestep must already be in ``_t_dev``.
        Returns float32 eps [B, out_channels, H, W].  Stream-ordered, allocation via torch only.

        ``control``: None, or the ControlNet residuals ``(down, mid, scales, skip_samples)``: ``down`` twelve channels-last tensors
        [Br, h*w, C] in the order of the skips, ``mid`` [Br, h*w, C] of the mid block's output, all UNSCALED and in the UNet dtype;
        ``scales`` the float32 device array of thirteen factors (hip_ops.CONTROL_RESIDUALS; index 12 is the mid residual's);
        ``skip_samples`` = B - Br leading samples that get no residual (guess mode: the unconditional half; the kernel's ``r_row0`` is
        that many samples' rows at each level).  Each residual is added where its skip is read: ``concat_channels`` in front of an
        up-block resnet becomes ``concat_channels_add``, the first one also carrying the mid residual.  None: today's launches.

        ``ip``: None, or the image-prompt context of ``prepare_ip_context`` (B rows, ordered like ``encoder_hidden_states``): every
        cross-attention adds its image branch.  None: today's launches.

        ``cfg_shared``: classifier-free guidance evaluates the SAME latents twice and only the text conditioning differs
        (stable_diffusion_dual_unet.py:1045-1047 ``torch.cat([latents] * 2)``).  Nothing before the first cross-attention
        reads the conditioning, so conv_in, the first ResnetBlock2D and the first transformer's GroupNorm / proj_in / whole
        self-attention / cross-attention query are computed ONCE on the B/2 unique samples (x then has B/2 rows, B is still
        the row count of ``encoder_hidden_states`` and of the result) and duplicated there: the full-resolution
        self-attention -- the longest kernel of the forward -- runs at half the batch."""
        w = self._w
        c = self.config
        eps = c.norm_eps
        ehs = encoder_hidden_states
        # measurement hook (tools/timeline.py): device-time stamps at the block boundaries of this forward, into
        # self._stamp_buf[self._stamp_row[0], k]; None in every normal run
        sb = getattr(self, "_stamp_buf", None)
        sk = [0]

        def mark():
            if sb is not None:
                ops.stamp(sb, sk[0], self._stamp_row)
                sk[0] += 1

        mark()
        if ehs.dtype != self._dtype:
            raise HipExtensionError("encoder_hidden_states must already be in the UNet dtype (use prepare_context)")
        if cfg_shared and (B % 2 or not self.supports_cfg_shared()):
            raise HipExtensionError("cfg_shared needs an even batch and a transformer in the first down block")
        if ip is not None:
            self._check_ip(ip, B)
        if self._lora_raw is not None:
            self._ensure_lora()
        temb = self._time_embedding(w, B)
        Bc = B // 2 if cfg_shared else B  # rows currently carried (the unique half until the first cross-attention)
        x, skips, H, W = self._down_mid(w, x, B, Bc, H, W, temb, ehs, mark, ip=ip)
        if control is not None:
            c_down, c_mid, c_scales, c_skip = control
            if len(c_down) != len(skips) or len(skips) + 1 != ops.CONTROL_RESIDUALS:
                raise HipExtensionError(f"control: {len(c_down)} down residuals for {len(skips)} skips (the fused concat indexes "
                                        f"{ops.CONTROL_RESIDUALS} scales: twelve skips and the mid block)")
        fu = self._freeu_table() if self._freeu is not None else None
        for i, blk in enumerate(w["up"]):
            fu_i = fu if i < 2 else None  # diffusers: the up blocks of resolution_idx 0 and 1, in front of each of their resnets
            for j, r in enumerate(blk["res"]):
                s, _, _ = skips.pop()
                if control is None and fu_i is not None:  # table [s1, s2, b1, b2]: stage i scales the backbone by b_i, filters with s_i
                    xs = ops.concat_channels_freeu(x, s, B, H, W, fu_i, 2 + i, i)
                elif control is None:
                    xs = ops.concat_channels(x, s)
                else:  # skip + residual where the skip is read; the mid residual rides on x in the first of them (used once)
                    k = len(skips)
                    xs = ops.concat_channels_add(x, s, ra=c_mid, rb=c_down[k], ia=ops.CONTROL_RESIDUALS - 1, ib=k, scales=c_scales,
                                                 r_row0=c_skip * H * W, hw=H * W if self._wants_colstats(H, W) else None)
                    c_mid = None
                    if fu_i is not None:  # diffusers adds the residuals before the up blocks: the filter sees the sums -- in place
                        ca = x.shape[-1]
                        xs = ops.concat_channels_freeu(xs[..., :ca], xs[..., ca:], B, H, W, fu_i, 2 + i, i, out=xs)
                x = self._resnet(r, xs, B, H, W, temb, eps)
                if "attn" in blk:
                    x = self._transformer(blk["attn"][j], x, B, H, W, ehs, ip=ip)
            if "us" in blk:
                # upsample to the size of the skip this level's output meets next (diffusers: upsample_size =
                # down_block_res_samples[-1].shape[2:]): 2H x 2W -- then the very launch of upsample=True -- unless the stride-2
                # convolution on the way down halved an odd side
                ho, wo = skips[-1][1:]
                cs = self._wants_colstats(ho, wo)
                if "us4" in blk and ops.upsample_phases_ok(self._dtype, B, H, W, x.shape[-1], blk["us4"].shape[1], (ho, wo), colstats=cs):
                    x, H, W = ops.conv3x3_up2(x, blk["us4"], B, H, W, bias=blk["us"][1], colstats=cs)
                else:
                    x, H, W = ops.conv3x3(x, blk["us"][0], B, H, W, bias=blk["us"][1], out_size=(ho, wo), colstats=cs)
            mark()  # end of an up block
        x = ops.groupnorm(x, B, c.norm_num_groups, w["norm_out"][0], w["norm_out"][1], eps, silu=True, split_out=self._sa(w["conv_out"][0]))
        y, _, _ = ops.conv3x3(x, w["conv_out"][0], B, H, W, bias=w["conv_out"][1], out_dtype=torch.float32)
        out = ops.unpack_nchw(y, B, c.out_channels, H, W)
        mark()  # end of the forward
        return out

    @_in_own_f32_mode
    def graphed_forward(self, B, H, W, ehs, cfg_shared=False, co_run=False, control=None, ip=None):
        """Capture ``forward_packed`` for this (batch, latent size) into a HIP graph (one per shape, cached).
        ``co_run``: the replays share the chip with another stream's forward (the dual-UNet pipeline's two streams): the launches are
        captured under the co-running plan family (``hip_ops.plan_family``, gmd_gemm_plan_family) -- a separate cache entry.
        Returns an object with ``.x`` (static packed-input buffer: fill it with ``pack_input(..., out=g.x)``) and
        ``.replay()`` -> float32 eps [B, out_channels, H, W] (static output buffer).  The timestep is read from the
        device scalar written by ``set_timestep``; the text conditioning from the in-place K / V^T buffers written by
        ``update_context`` -- both outside the graph, so one capture serves every step and every prompt.
        ``control`` (see forward_packed): the graph reads the ControlNet's static residual buffers and the device array of scales, so
        the key gains their identity; None is today's key and today's graph.
        ``ip`` (see forward_packed): the graph reads the persistent K_ip / V_ip^T buffers of (rows, Nip) and the device array of
        scales, so the key gains ("ip", rows, Nip): one capture serves every image and every scale."""
        self._ensure()
        self.update_context(ehs)
        if self.config.addition_embed_type is not None and B not in self._aug:
            raise HipExtensionError("set_added_cond(added_cond_kwargs, batch) must precede graphed_forward for this UNet")
        if self.config.time_cond_proj_dim is not None:
            self._tcond_entry(B)  # exists (zeros unless set_timestep_cond wrote it) before the capture reads it
        key = (B, H, W, tuple(ehs.shape), bool(cfg_shared), bool(co_run))
        if control is not None:
            key += (tuple(t.data_ptr() for t in control[0]) + (control[1].data_ptr(), control[2].data_ptr(), int(control[3])),)
        if ip is not None:
            self._check_ip(ip, B)
            key += (("ip", ip.rows, ip.nip),)
        if self._lora_raw is not None:  # the graph holds the adapter's launches and reads its factors and its table of scales
            self._ensure_lora()
            key += (("lora", self._lora_id),)
        if self._freeu is not None:  # other launches; the numbers are read from the device table, so one graph serves every setting
            self._freeu_table()
            key += (("freeu",),)
        g = self._graphs.get(key)
        if g is not None:
            return g
        from .. import profiling

        if profiling.active() is not None:
            raise HipExtensionError("graph capture with an active KernelTimer is not supported")
        g = _GraphedForward()
        g.x = torch.empty((B // 2 if cfg_shared else B, H * W, self._cin_pad), dtype=self._dtype, device=self._device)
        g.x.zero_()
        g.control = control  # the captured launches read these buffers: alive as long as the graph
        cur = torch.cuda.current_stream(self._device)
        side = torch.cuda.Stream(device=self._device)
        side.wait_stream(cur)
        with torch.cuda.stream(side), ops.plan_family(co_run):  # warm-up on a side stream: one-time attribute calls, workspaces, allocator pools
            for _ in range(2):
                self.forward_packed(g.x, B, H, W, ehs, cfg_shared=cfg_shared, control=control, ip=ip)
        cur.wait_stream(side)
        torch.cuda.synchronize(self._device)
        g.graph = torch.cuda.CUDAGraph()
        g.ws = ops.new_workspace(self._device)  # this graph's own split-K scratch (see hip_ops.workspace_scope)
        self._capturing = True
        try:
            with ops.capture_in_flight(), ops.workspace_scope(g.ws), ops.plan_family(co_run), torch.cuda.graph(g.graph):
                g.out = self.forward_packed(g.x, B, H, W, ehs, cfg_shared=cfg_shared, control=control, ip=ip)
        finally:
            self._capturing = False
        while len(self._graphs) >= self.max_cached_graphs:  # oldest first: a graph pins its activations pool and 96 MB of scratch
            self._graphs.pop(next(iter(self._graphs)))
        self._graphs[key] = g
        return g

    @_in_own_f32_mode
    def prepare_context(self, encoder_hidden_states):
        """Cast text-encoder hidden states to the UNet dtype once (HIP cast kernel)."""
        self._ensure()
        ehs = encoder_hidden_states
        if not ehs.is_cuda:
            raise HipExtensionError("encoder_hidden_states must be on the HIP device")
        ehs = ehs.contiguous()
        if ehs.dtype == self._dtype:
            return ehs
        if ehs.dtype not in (torch.float32, torch.bfloat16, torch.float16):
            ehs = ehs.float()
        return ops.cast(ehs, self._dtype)

    def pack_input(self, sample, dup=1, out=None, div=None):
        """sample: float32 NCHW tensor, or a tuple ``(cond, x)`` concatenated on channels (conditioning first:
        stable_diffusion_gm.py:1045, dual_unet.py:1080); dup=2 duplicates the batch for CFG (gm.py:1047).  ``div``: None, or the
        float32 divisors ``(d_cond, d_x)`` of the two parts (a single tensor takes a number or ``(d, 1.0)``): a sigma-space
        scheduler's ``scale_model_input`` folded into the pack (gm.py:1048)."""
        self._ensure()
        a, b = (sample if isinstance(sample, (tuple, list)) else (sample, None))
        if a.dtype != torch.float32:
            a = ops.cast(a.contiguous(), torch.float32)
        if b is not None and b.dtype != torch.float32:
            b = ops.cast(b.contiguous(), torch.float32)
        nch = a.shape[1] + (0 if b is None else b.shape[1])
        if nch != self.config.in_channels:
            raise ValueError(f"UNet expects {self.config.in_channels} input channels, got {nch}")
        if div is None:
            return ops.pack_unet_input(a.contiguous(), None if b is None else b.contiguous(), dup, self._cin_pad, self._dtype, out=out)
        div = tuple(div) if isinstance(div, (tuple, list)) else (div, 1.0)
        return ops.pack_unet_input(a.contiguous(), None if b is None else b.contiguous(), dup, self._cin_pad, self._dtype, out=out, div=div)

    def _control_from_nchw(self, down, mid, B):
        """diffusers' ``down_block_additional_residuals`` / ``mid_block_additional_residual`` (NCHW, already scaled by the ControlNet)
        as the ``control`` of forward_packed: channels-last in the UNet dtype, every scale 1 (``s + r * 1`` is ``s + r``)."""
        if down is None or mid is None:
            raise ValueError("down_block_additional_residuals and mid_block_additional_residual must be given together")

        def cl(t):
            if not torch.is_tensor(t) or t.dim() != 4 or t.shape[0] != B or not t.is_cuda:
                raise ValueError(f"additional residuals must be device tensors [B={B}, C, h, w]")
            t = t.permute(0, 2, 3, 1).reshape(B, t.shape[2] * t.shape[3], t.shape[1]).contiguous()
            if t.dtype != self._dtype:
                t = ops.cast(t if t.dtype in (torch.float32, torch.bfloat16, torch.float16) else t.float(), self._dtype)
            return t

        ones = torch.ones(ops.CONTROL_RESIDUALS, dtype=torch.float32, device=self._device)
        return ([cl(t) for t in down], cl(mid), ones, 0)

    @_in_own_f32_mode
    def __call__(self, sample, timestep, encoder_hidden_states=None, timestep_cond=None, cross_attention_kwargs=None,
                 added_cond_kwargs=None, down_block_additional_residuals=None, mid_block_additional_residual=None,
                 return_dict=True, **kwargs):
        if timestep_cond is not None and self.config.time_cond_proj_dim is None:
            raise ValueError("timestep_cond was given, but this UNet has no time_embedding.cond_proj: its config key "
                             "time_cond_proj_dim is None")
        self._ensure()
        first = sample[0] if isinstance(sample, (tuple, list)) else sample
        B, _, H, W = first.shape
        x = self.pack_input(sample)
        ehs = self.prepare_context(encoder_hidden_states)
        if ehs.shape[0] != B:
            raise ValueError(f"encoder_hidden_states batch {ehs.shape[0]} != sample batch {B}")
        self.set_timestep(timestep)
        ip = None
        if added_cond_kwargs and "image_embeds" in added_cond_kwargs:  # diffusers' form: a list with one tensor per adapter
            added_cond_kwargs = dict(added_cond_kwargs)
            ip = self.prepare_ip_context(self._single_adapter_embeds(added_cond_kwargs.pop("image_embeds")))
        self.set_added_cond(added_cond_kwargs, B)
        if self.config.time_cond_proj_dim is not None:
            self.set_timestep_cond(None if timestep_cond is None else timestep_cond.to(self._device), B)
        if down_block_additional_residuals is None and mid_block_additional_residual is None:
            out = self.forward_packed(x, B, H, W, ehs, ip=ip)
        else:
            out = self.forward_packed(x, B, H, W, ehs, ip=ip, control=self._control_from_nchw(down_block_additional_residuals,
                                                                                            mid_block_additional_residual, B))
        if not return_dict:
            return (out,)
        from .image_processor import UNetOutput

        return UNetOutput(sample=out)

    forward = __call__
