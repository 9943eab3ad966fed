"""
``ControlNetModel`` for the MI355X build: diffusers' SD-1.5 ControlNet (``lllyasviel/sd-controlnet-*``, ``control_v11*``) on the
hand-written HIP kernels -- the conditioning the reference gets from diffusers for its "ControlNet-conditioned HDR generation"
experiment (the SDR UNet steered by an edge / depth / pose map; the gain-map UNet follows the SDR x0 and is never conditioned).

A ControlNet is a copy of its UNet's encoder (conv_in, time embedding, down blocks, mid block) plus
  * ``controlnet_cond_embedding``: conv 3->e0, (e_i->e_i, e_i->e_{i+1} stride 2) x 3, each followed by SiLU, then conv e3->C0 -- the
    conditioning image (8x the latent side) brought to the latent grid, ADDED to conv_in's output;
  * thirteen zero convolutions (1x1): one per skip tensor of the encoder and one for the mid block's output.
The encoder half is the UNet's own code: the weights are prepared by ``UNet2DConditionModel._prepare_encoder`` and the walk is
``UNet2DConditionModel._down_mid`` -- the same launches, layouts and plans.  The conditioning embedding runs ONCE per call
(``set_condition``: gmd_conv3x3 + gmd_silu) into a persistent buffer that conv_in takes as its epilogue residual; the zero convolutions
are gmd_gemm_nt launches into thirteen channels-last buffers, UNSCALED: the consumer (gmd_concat_channels_add in the UNet's up blocks)
applies ``scales[i]`` from device memory, so a captured graph serves every ``controlnet_conditioning_scale``.

State-dict keys follow diffusers.  Not built: Multi-ControlNet, ``global_pool_conditions``, a "bgr" channel order, the CFG shared
prefix inside the ControlNet.
"""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Any

import torch

from .. import hip_ops as ops
from .._native import HipExtensionError
from .configuration import read_state_dict
from .image_processor import _Output
from .unet_2d_condition import SD15_UNET_DEFAULTS, UNet2DConditionModel, _GraphedForward, _HipModule, _in_own_f32_mode, _pad_to

_U = UNet2DConditionModel

# the UNet config keys a ControlNet shares with it (its encoder), then its own
_ENCODER_KEYS = ("in_channels", "flip_sin_to_cos", "freq_shift", "down_block_types", "block_out_channels", "layers_per_block",
                 "downsample_padding", "mid_block_scale_factor", "act_fn", "norm_num_groups", "norm_eps", "cross_attention_dim",
                 "attention_head_dim", "transformer_layers_per_block", "use_linear_projection")
CONTROLNET_DEFAULTS = dict({k: SD15_UNET_DEFAULTS[k] for k in _ENCODER_KEYS}, conditioning_channels=3,
                           conditioning_embedding_out_channels=(16, 32, 96, 256), controlnet_conditioning_channel_order="rgb",
                           global_pool_conditions=False,
                           # read by the shared encoder code; an SD-1.5 ControlNet has neither (anything else is refused)
                           addition_embed_type=None, time_cond_proj_dim=None)
_ONLY = dict(controlnet_conditioning_channel_order="rgb", global_pool_conditions=False)  # the only values implemented


@dataclass
class ControlNetOutput(_Output):
    down_block_res_samples: Any
    mid_block_res_sample: torch.Tensor


def control_window(i, n, start=0.0, end=1.0):
    """diffusers' ``controlnet_keep`` for step ``i`` of ``n``: the ControlNet runs unless the step lies outside [start, end]."""
    return not (i / n < start or (i + 1) / n > end)


def control_scales(scale=1.0, guess_mode=False):
    """The thirteen factors of the residuals (twelve down, then mid) as a host float32 tensor: ``scale`` everywhere, or diffusers'
    guess-mode ramp ``logspace(-1, 0, 13) * scale`` (0.1 at the first skip, 1 at the mid block)."""
    n = ops.CONTROL_RESIDUALS
    if guess_mode:
        return torch.logspace(-1, 0, n) * scale
    return torch.full((n,), float(scale), dtype=torch.float32)


class ControlNetModel(_HipModule):
    config_name = "config.json"
    max_cached_graphs = 8
    _defaults = CONTROLNET_DEFAULTS

    # the encoder half is the UNet's code, method for method (nothing here restates a launch)
    _prepare_encoder = _U._prepare_encoder
    _sa = staticmethod(_U._sa)
    _wants_colstats = staticmethod(_U._wants_colstats)
    _dup_batch = staticmethod(_U._dup_batch)
    _resnet = _U._resnet
    _self_attention = _U._self_attention
    _cross_kv = _U._cross_kv
    _transformer = _U._transformer
    _transformer_block = _U._transformer_block
    _time_embedding = _U._time_embedding
    _down_mid = _U._down_mid
    update_context = _U.update_context
    prepare_context = _U.prepare_context
    set_timestep = _U.set_timestep
    set_timestep_from = _U.set_timestep_from
    pack_input = _U.pack_input

    def __init__(self, **config):
        cfg = dict(CONTROLNET_DEFAULTS)
        unknown = [k for k in config if k not in cfg and not k.startswith("_")]
        cfg.update({k: v for k, v in config.items() if k in cfg})
        if "num_attention_heads" in config and config["num_attention_heads"] is not None:
            cfg["attention_head_dim"] = config["num_attention_heads"]
        for k, only in _ONLY.items():
            if cfg[k] != only:
                raise NotImplementedError(f"{k}={cfg[k]!r}: only {k}={only!r} is implemented")
        for k in ("class_embed_type", "addition_embed_type", "num_class_embeds", "time_cond_proj_dim"):
            if config.get(k) is not None:
                raise NotImplementedError(f"{k}={config[k]!r}: only SD-1.5 ControlNets (no class / added / guidance embedding) are implemented")
        oca = config.get("only_cross_attention", False)
        if any(oca) if isinstance(oca, (list, tuple)) else oca:
            raise NotImplementedError(f"only_cross_attention={oca!r}")
        cfg["conditioning_embedding_out_channels"] = tuple(cfg["conditioning_embedding_out_channels"])
        if len(cfg["conditioning_embedding_out_channels"]) < 1 or cfg["conditioning_channels"] < 1:
            raise ValueError("conditioning_embedding_out_channels / conditioning_channels must be non-empty / positive")
        self._unknown_config = unknown
        self.register_to_config(**cfg)
        self._encoder = self._as_unet()  # weightless: the structure (and the refusals) of the UNet this ControlNet copies
        self._init_module()
        self._kv_cache = {}
        self._t_dev = None
        self._capturing = False
        self._transformers = []
        self._graphs = {}
        self._aug = {}
        self._tcond = {}
        self._cond = {}        # (B, h, w) -> persistent channels-last [B, h*w, C0] conditioning embedding, rewritten in place
        self._scales_dev = None

    # ------------------------------------------------------------------------------------------
    # structure
    # ------------------------------------------------------------------------------------------
    def _as_unet(self):
        """A weightless ``UNet2DConditionModel`` with this ControlNet's encoder configuration."""
        cfg = {k: self.config[k] for k in _ENCODER_KEYS}
        n = len(cfg["block_out_channels"])
        return UNet2DConditionModel(**cfg, up_block_types=("UpBlock2D",) * n, out_channels=cfg["in_channels"])

    def _layout(self):
        return self._encoder._layout()

    def skip_channels(self):
        """Channels of the encoder's skip tensors, in diffusers' ``down_block_res_samples`` order (twelve for SD-1.5)."""
        ch = list(self.config.block_out_channels)
        out = [ch[0]]
        for i in range(len(ch)):
            out += [ch[i]] * self.config.layers_per_block
            if i != len(ch) - 1:
                out.append(ch[i])
        return out

    def expected_keys(self):
        keys = {k: v for k, v in self._encoder.expected_keys().items()
                if k.startswith(("conv_in.", "time_embedding.", "down_blocks.", "mid_block."))}

        def conv(k, co, ci, ks):
            keys[k + ".weight"], keys[k + ".bias"] = (co, ci, ks, ks), (co,)

        e = list(self.config.conditioning_embedding_out_channels)
        ch = list(self.config.block_out_channels)
        conv("controlnet_cond_embedding.conv_in", e[0], self.config.conditioning_channels, 3)
        for i in range(len(e) - 1):
            conv(f"controlnet_cond_embedding.blocks.{2 * i}", e[i], e[i], 3)
            conv(f"controlnet_cond_embedding.blocks.{2 * i + 1}", e[i + 1], e[i], 3)
        conv("controlnet_cond_embedding.conv_out", ch[0], e[-1], 3)
        for i, c in enumerate(self.skip_channels()):
            conv(f"controlnet_down_blocks.{i}", c, c, 1)
        conv("controlnet_mid_block", ch[-1], ch[-1], 1)
        return keys

    @staticmethod
    def _is_zero_conv(k):
        return k.startswith(("controlnet_down_blocks.", "controlnet_mid_block.", "controlnet_cond_embedding.conv_out."))

    # ------------------------------------------------------------------------------------------
    # loading
    # ------------------------------------------------------------------------------------------
    @classmethod
    def from_pretrained(cls, path, subfolder=None, torch_dtype=None):
        """Read a diffusers-layout directory (``config.json`` + ``diffusion_pytorch_model.safetensors``)."""
        d = os.path.join(path, subfolder) if subfolder else path
        m = cls(**cls.load_config(d))
        m.load_state_dict(read_state_dict(d))
        if torch_dtype is not None:
            m.to(torch_dtype)
        return m

    def save_pretrained(self, directory):
        import json
        from safetensors.torch import save_file

        os.makedirs(directory, exist_ok=True)
        with open(os.path.join(directory, "config.json"), "w") as f:
            json.dump({"_class_name": "ControlNetModel", **{k: (list(v) if isinstance(v, tuple) else v) for k, v in self.config.items()}}, f, indent=2)
        save_file({k: v.contiguous() for k, v in self._raw.items()}, os.path.join(directory, "diffusion_pytorch_model.safetensors"))

    def _draw(self, keys, seed, zero, device=None):
        g = torch.Generator(device or "cpu").manual_seed(seed)
        want = self.expected_keys()
        sd = {}
        for k in keys:
            shp = want[k]
            if zero(k):
                sd[k] = torch.zeros(shp)
            elif ".norm" in k or k.endswith(("norm.weight", "norm.bias")):
                sd[k] = torch.ones(shp) if k.endswith("weight") else torch.zeros(shp)
            else:
                fan_in = 1
                for s_ in want[k.rsplit(".", 1)[0] + ".weight"][1:]:
                    fan_in *= s_
                sd[k] = (torch.rand(shp, generator=g, device=g.device) * 2 - 1) * fan_in ** -0.5
        return sd

    @classmethod
    def from_unet(cls, unet, conditioning_embedding_out_channels=(16, 32, 96, 256), conditioning_channels=3, seed=0):
        """diffusers' ``ControlNetModel.from_unet``: the UNet's encoder weights copied, the zero convolutions (and the embedding's
        conv_out) zero, the rest of the conditioning embedding drawn afresh -- a ControlNet whose residuals are all zero."""
        m = cls(**{k: unet.config[k] for k in _ENCODER_KEYS}, conditioning_embedding_out_channels=conditioning_embedding_out_channels,
                conditioning_channels=conditioning_channels)
        want = m.expected_keys()
        src = unet.state_dict()
        sd = {k: src[k].clone() for k in want if k in src}
        sd.update(m._draw([k for k in want if k not in sd], seed, m._is_zero_conv))
        m.load_state_dict(sd)
        return m.to(unet.device, unet.dtype)

    def init_random(self, seed=1234, device=None):
        """Deterministic synthetic weights as ``UNet2DConditionModel.init_random``, the zero convolutions included (NON-zero): tests
        and benchmarks; no checkpoint exists offline.  ``device``: draw with that device's generator (other values, much faster)."""
        return self.load_state_dict(self._draw(list(self.expected_keys()), seed, lambda k: False, device))

    # ------------------------------------------------------------------------------------------
    # weight preparation
    # ------------------------------------------------------------------------------------------
    def _conv3_padded(self, key, cin_pad, cout_pad):
        """A conditioning-embedding convolution with BOTH channel counts zero-padded to what gmd_conv3x3 reads next: the padded output
        channels are exactly zero (zero rows, zero bias) and stay zero through the SiLU."""
        w, b = self._raw[key + ".weight"], self._raw[key + ".bias"]
        cout, cin = w.shape[0], w.shape[1]
        t = torch.zeros(cout_pad, 3, 3, cin_pad)
        t[:cout, ..., :cin] = w.permute(0, 2, 3, 1)
        bp = torch.zeros(cout_pad)
        bp[:cout] = b
        return self._wt(t.reshape(cout_pad, 9 * cin_pad)), self._f32(bp)

    def _prepare(self):
        c = self.config
        w = {}
        _, _, te_w, te_b = self._prepare_encoder(w)
        w["te_all"] = (self._wt(torch.cat(te_w, 0)), self._f32(torch.cat(te_b, 0)))
        km = self._kmul()
        e = list(c.conditioning_embedding_out_channels)
        names = ["conv_in"] + [f"blocks.{i}" for i in range(2 * (len(e) - 1))]
        couts = [e[i // 2] for i in range(len(names))]  # conv_in e0; blocks 2k: e_k -> e_k, blocks 2k+1: e_k -> e_{k+1} (stride 2)
        self._cond_cin_pad = cin = _pad_to(c.conditioning_channels, km)
        emb = []
        for i, (nm, co) in enumerate(zip(names, couts)):
            cop = _pad_to(co, km)
            emb.append(self._conv3_padded("controlnet_cond_embedding." + nm, cin, cop) + (2 if (i and i % 2 == 0) else 1,))
            cin = cop
        w["emb"] = emb  # (weight, bias, stride): conv_in, then (same width, stride 2 to the next width) per level
        w["emb_out"] = self._conv3_padded("controlnet_cond_embedding.conv_out", cin, c.block_out_channels[0])
        w["zero"] = [self._lin(f"controlnet_down_blocks.{i}") for i in range(len(self.skip_channels()))]
        w["zero_mid"] = self._lin("controlnet_mid_block")
        self._kv_cache = {}
        self._graphs = {}
        self._aug = {}
        self._tcond = {}
        self._cond = {}
        self._t_dev = torch.zeros(1, dtype=torch.float32, device=self._device)
        self._scales_dev = torch.ones(ops.CONTROL_RESIDUALS, dtype=torch.float32, device=self._device)
        return w

    # ------------------------------------------------------------------------------------------
    # forward
    # ------------------------------------------------------------------------------------------
    def set_scales(self, scale=1.0, guess_mode=False):
        """Write the thirteen residual factors into the device array the UNet's fused concat reads (outside any captured graph, as the
        timestep scalar is: one graph serves every ``controlnet_conditioning_scale``).  Returns the device array."""
        self._ensure()
        self._scales_dev.copy_(control_scales(scale, guess_mode), non_blocking=False)
        return self._scales_dev

    @_in_own_f32_mode
    def set_condition(self, image, B):
        """Run the conditioning embedding once per call: ``image`` float32 NCHW [B, conditioning_channels, 8h, 8w] on the device, values
        as diffusers' control-image processor leaves them ([0, 1], no normalisation) -> the persistent channels-last buffer
        [B, h*w, C0] that conv_in adds in its epilogue.  Later calls rewrite the buffer in place, outside any graph."""
        self._ensure()
        c = self.config
        if not torch.is_tensor(image) or image.dim() != 4 or image.shape[0] != B or image.shape[1] != c.conditioning_channels:
            raise ValueError(f"controlnet_cond must be a tensor [{B}, {c.conditioning_channels}, H, W]; got "
                             f"{tuple(image.shape) if torch.is_tensor(image) else type(image).__name__}")
        down = 2 ** (len(c.conditioning_embedding_out_channels) - 1)
        if image.shape[2] % down or image.shape[3] % down:
            raise ValueError(f"controlnet_cond sides must be multiples of {down} (the conditioning embedding halves them "
                             f"{len(c.conditioning_embedding_out_channels) - 1} times); got {tuple(image.shape[2:])}")
        if not image.is_cuda:
            raise HipExtensionError("controlnet_cond must be on the HIP device")
        if self._capturing:
            raise HipExtensionError("the conditioning embedding must be prepared (set_condition) before graph capture")
        w = self._w
        img = image.contiguous()
        if img.dtype != torch.float32:
            img = ops.cast(img if img.dtype in (torch.bfloat16, torch.float16) else img.float(), torch.float32)
        H, W = img.shape[2], img.shape[3]
        x = ops.pack_unet_input(img, None, 1, self._cond_cin_pad, self._dtype)
        for wt, b, stride in w["emb"]:
            x, H, W = ops.conv3x3(x, wt, B, H, W, bias=b, stride=stride)
            ops.silu_(x)
        x, H, W = ops.conv3x3(x, w["emb_out"][0], B, H, W, bias=w["emb_out"][1])
        buf = self._cond.get((B, H, W))
        if buf is None:
            self._cond[(B, H, W)] = buf = x
        else:
            buf.copy_(x)  # in place: a captured graph keeps reading this buffer
        return buf

    @_in_own_f32_mode
    def forward_packed(self, x, B, H, W, encoder_hidden_states):
        """x: packed channels-last latents [B, H*W, cin_pad]; the timestep in ``_t_dev``, the conditioning embedding in its buffer
        (``set_condition``).  Returns (down, mid): twelve channels-last residuals [B, h*w, C] in the order of the UNet's skips and the
        mid-block residual, UNSCALED, in the model dtype."""
        w = self._w
        ehs = encoder_hidden_states
        if ehs.dtype != self._dtype:
            raise HipExtensionError("encoder_hidden_states must already be in the ControlNet dtype (use prepare_context)")
        cond = self._cond.get((B, H, W))
        if cond is None:
            raise HipExtensionError(f"no conditioning embedding for batch {B} at {H}x{W}: call set_condition(image, batch) first")
        temb = self._time_embedding(w, B)
        x, skips, H, W = self._down_mid(w, x, B, B, H, W, temb, ehs, lambda: None, cond=cond)
        if len(skips) != len(w["zero"]):
            raise HipExtensionError("the encoder produced a different number of skips than there are zero convolutions")
        down = []
        for (s, h_, w_), (zw, zb) in zip(skips, w["zero"]):
            C = s.shape[-1]
            down.append(ops.gemm_nt(s.view(B * h_ * w_, C), zw, bias=zb).view(B, h_ * w_, C))
        C = x.shape[-1]
        mid = ops.gemm_nt(x.view(B * H * W, C), w["zero_mid"][0], bias=w["zero_mid"][1]).view(B, H * W, C)
        return down, mid

    @_in_own_f32_mode
    def graphed_forward(self, B, H, W, ehs, co_run=False):
        """Capture ``forward_packed`` into a HIP graph (one per shape, cached), as the UNet's: own workspace, plan family.  The result
        has ``.x`` (static packed input), ``.replay()`` and the static outputs ``.down`` (twelve buffers) / ``.mid``."""
        self._ensure()
        self.update_context(ehs)
        if (B, H, W) not in self._cond:
            raise HipExtensionError("set_condition(image, batch) must precede graphed_forward")
        key = (B, H, W, tuple(ehs.shape), bool(co_run))
        g = self._graphs.get(key)
        if g is not None:
            return g
        from .. import profiling

        if profiling.active() is not None:
            raise HipExtensionError("graph capture with an active KernelTimer is not supported")
        g = _GraphedForward()
        g.x = torch.zeros((B, H * W, self._cin_pad), dtype=self._dtype, device=self._device)
        cur = torch.cuda.current_stream(self._device)
        side = torch.cuda.Stream(device=self._device)
        side.wait_stream(cur)
        with torch.cuda.stream(side), ops.plan_family(co_run):
            for _ in range(2):
                self.forward_packed(g.x, B, H, W, ehs)
        cur.wait_stream(side)
        torch.cuda.synchronize(self._device)
        g.graph = torch.cuda.CUDAGraph()
        g.ws = ops.new_workspace(self._device)
        self._capturing = True
        try:
            with ops.capture_in_flight(), ops.workspace_scope(g.ws), ops.plan_family(co_run), torch.cuda.graph(g.graph):
                g.down, g.mid = self.forward_packed(g.x, B, H, W, ehs)
        finally:
            self._capturing = False
        g.out = (g.down, g.mid)
        while len(self._graphs) >= self.max_cached_graphs:
            self._graphs.pop(next(iter(self._graphs)))
        self._graphs[key] = g
        return g

    @_in_own_f32_mode
    def __call__(self, sample, timestep, encoder_hidden_states, controlnet_cond, conditioning_scale=1.0, guess_mode=False,
                 return_dict=True):
        """diffusers' ``ControlNetModel.forward``: NCHW residuals in the model dtype, already scaled (guess mode:
        ``logspace(-1, 0, 13) * conditioning_scale``).  The slow parity path: the pipelines' fused loop hands the UNSCALED
        channels-last buffers to the UNet, whose concat kernel applies the scale."""
        self._ensure()
        B, _, H, W = sample.shape
        x = self.pack_input(sample)
        ehs = self.prepare_context(encoder_hidden_states)
        if ehs.shape[0] != B:
            raise ValueError(f"encoder_hidden_states batch {ehs.shape[0]} != sample batch {B}")
        self.set_timestep(timestep)
        self.set_condition(controlnet_cond, B)
        down, mid = self.forward_packed(x, B, H, W, ehs)
        sc = [float(v) for v in control_scales(conditioning_scale, guess_mode)]
        hw = []
        h_, w_ = H, W
        for blk in self._w["down"]:
            hw += [(h_, w_)] * len(blk["res"])
            if "ds" in blk:
                h_, w_ = (h_ + 1) // 2, (w_ + 1) // 2
                hw.append((h_, w_))
        hw = [(H, W)] + hw

        def nchw(t, s, size):
            return (t * s).view(B, size[0], size[1], t.shape[-1]).permute(0, 3, 1, 2).contiguous()

        down = [nchw(t, s, z) for t, s, z in zip(down, sc, hw)]
        mid = nchw(mid, sc[-1], (h_, w_))
        if not return_dict:
            return (down, mid)
        return ControlNetOutput(down_block_res_samples=down, mid_block_res_sample=mid)

    forward = __call__
