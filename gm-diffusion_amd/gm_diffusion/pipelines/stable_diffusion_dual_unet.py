# Portions of this file keep API-surface text (the ``__call__`` / constructor signatures, ``encode_prompt``, ``check_inputs``
# error messages, the property block and the output tail) of diffusers' ``StableDiffusionPipeline``, which the reference's
# pipeline files are copies of with ~40 changed lines each (their header, reproduced as the Apache License 2.0 requires):
#
#     Copyright 2024 The HuggingFace Team. All rights reserved.
#
#     Licensed under the Apache License, Version 2.0 (the "License");
#     you may not use this file except in compliance with the License.
#     You may obtain a copy of the License at
#
#         http://www.apache.org/licenses/LICENSE-2.0
#
#     Unless required by applicable law or agreed to in writing, software
#     distributed under the License is distributed on an "AS IS" BASIS,
#     WITHOUT WARRANTIES OR CONDITIONS OF ANY KIND, either express or implied.
#     See the License for the specific language governing permissions and
#     limitations under the License.
#
# Changes from that text: the LoRA / textual-inversion branches are removed, the IP-adapter branch keeps the plain adapter only, the
# denoising loop, latent step, UNet / VAE calls and the decode tail are new (hand-written HIP kernels behind gm_diffusion.hip_ops; see
# DESIGN.md).
"""
``StableDiffusionDualUNetPipeline`` -- the Stage-3 text->HDR path: an SDR UNet (with
classifier-free guidance) and a GM UNet (conditional only, fed the SDR x0-prediction) are stepped
jointly with two scheduler instances.  Drop-in mirror of the reference class at
gm_diffusion/pipelines/stable_diffusion_dual_unet.py:156 (constructor :202-214, ``__call__``
:782-1140).

Per iteration (reference lines):
  1045-1060  SDR UNet on cat([latents]*2)                      -> pack kernel (CFG duplicate) + HIP UNet
  1063-1069  CFG combine (+ rescale_noise_cfg)                 \\
  1071-1075  x0 = (x - sqrt(1-a) eps) / sqrt(a)                  > ONE fused HIP kernel (gmd_latent_step)
  1077       latents = scheduler.step(eps, t, latents)         /
  1080       gm_in = cat([x0, gm_latents], dim=1)              -> folded into the GM UNet input pack
  1083-1092  GM UNet on gm_in with the conditional embeddings  -> HIP UNet
  1093       gm_latents = gm_scheduler.step(...)               -> gmd_latent_step (no CFG)

Generalisations over the reference as written: the GM UNet receives the
conditional half ``prompt_embeds[negative.shape[0]:]`` (scripts/inference/experiments/
visualize_latents.py:274), which equals the reference's ``prompt_embeds[1:]`` for its only working
case (batch 1 + CFG) and also works for batch > 1 and without CFG; with a non-latent
``output_type`` BOTH latents are decoded (the reference decodes neither correctly,
dual_unet.py:1117-1132).  As in the reference the result is always the bare tuple
``(sdr, gm)`` and ``return_dict`` is ignored (:1132); ``callback_on_step_end`` is accepted and
ignored (:1095-1103 is commented out there).

Sigma-space schedulers (``EulerDiscreteScheduler``, ``EulerAncestralDiscreteScheduler``, ``LMSDiscreteScheduler``): the reference cannot run one here -- its loop
indexes ``alphas_cumprod`` with the (float) timestep (:1072) and overwrites the GM state with its scaled copy (:1048) -- so, unlike the
GM pipeline (which mirrors the reference and divides the whole concatenated input, stable_diffusion_gm.py:1048), this pipeline defines
the behaviour by the mathematics: the SDR UNet input is ``latents / (sigma**2 + 1) ** 0.5``; ``x0_latent`` is the scheduler's
``pred_original_sample`` ``x - sigma * eps`` (the VP expression of :1075 in exact arithmetic); the GM UNet input is
``cat([x0_latent, gm_latents / (sigma**2 + 1) ** 0.5])`` with x0 undivided; neither state is ever scaled.  Fused device path only: the
generic loop raises a ValueError for such a scheduler.

Guidance-embedded (LCM) UNets (config ``time_cond_proj_dim``; :1024-1030): the SDR UNet takes the embedding of ``guidance_scale - 1``
as ``timestep_cond`` and runs without the CFG duplicate.  The reference hands that one tensor, of the SDR UNet's width, to BOTH UNets
(:1056, :1088), which only works when both have the same ``time_cond_proj_dim``.  Here the GM UNet gets an embedding of its own
width if and only if it has ``time_cond_proj_dim`` itself, and none otherwise: equal to the reference where the reference runs.

ControlNet (the reference README's "ControlNet-conditioned HDR generation", which it gets from diffusers): the constructor keyword
``controlnet=`` takes a ``components.ControlNetModel`` and ``__call__`` then reads diffusers' ``control_image``,
``controlnet_conditioning_scale``, ``guess_mode``, ``control_guidance_start`` / ``control_guidance_end``.  Only the SDR UNet is steered;
the GM UNet follows the SDR x0.  Fused path: inside the guidance window a step replays the ControlNet's graph and then the UNet's control
graph on the SDR stream, outside it the plain UNet graph; the scale lives in device memory, so no value of it needs a new capture.

IP-Adapter (:518-585, :986-1020, :1058): ``load_ip_adapter`` installs a plain adapter (4 image tokens per picture) from local files,
``ip_adapter_image`` / ``ip_adapter_image_embeds`` are prepared as in the reference ([negative; positive] rows, zeros as the negative
image embedding) and every cross-attention of the SDR UNet becomes the decoupled one (one launch, gmd_attention_ip).  The reference
hands the same ``added_cond_kwargs`` to both UNets (:1058, :1090), which only runs when both carry an adapter; here the GM UNet gets
the positive rows if and only if an adapter was loaded into it (``pipe.gm_unet.load_ip_adapter``).  The scale lives in device memory:
``set_ip_adapter_scale`` between two calls needs no new capture.  Plus / FaceID variants, several adapters, ``ip_adapter_masks`` and
per-block scales are refused by name.

img2img and inpainting (diffusers' ``image``, ``strength``, ``mask_image``; the reference has neither): reached only when ``image`` is
given.  Without it nothing changes, and ``mask_image`` or ``strength`` alone is a ValueError.
  ``image``       float tensor [1 | rows, 3, H, W] in [0, 1], or uint8 [.., H, W, 3] tensor / array / PIL image or a list of them
                  (``VaeImageProcessor.preprocess``: normalise and lay out only; another size than the call's is a ValueError, resize
                  with ``hdr.prepare_sdr``), or [1 | rows, 4, h, w] latents already multiplied by ``scaling_factor``.  rows = batch x
                  ``num_images_per_prompt``; one image is repeated.  Pixels become ``z0 = vae.encode(x).latent_dist.sample(generator)
                  * scaling_factor`` in float32.
  ``strength``    default 0.8, 1.0 with a mask; outside [0, 1] or ``int(num_inference_steps * strength) < 1`` is a ValueError.
  ``mask_image``  [1 | rows, 1, H, W] or [H, W]; float, uint8 (255 = 1) or PIL "L"; 1 = repaint, 0 = keep.  Binarised at 0.5 and
                  brought to latent size by ``F.interpolate`` (nearest), as diffusers' ``prepare_mask_latents``; a float mask
                  [1 | rows, 1, h, w] of latent size is taken as it is.  4-channel SDR UNets only.
Schedule (diffusers' ``get_timesteps``): ``t_start = max(N - min(int(N * strength), N), 0)``; the SDR branch runs
``timesteps[t_start * order:]`` and its scheduler gets ``set_begin_index(t_start * order)``.  ``LCMScheduler`` takes ``strength`` in
``set_timesteps`` instead and nothing is sliced.  ``noise = randn_tensor(latent shape, generator)`` (a given ``latents=`` is that
noise); the generator serves the encoder's sample (pixels only), then ``noise``, then the steps' own draws.  The SDR latents start as
``scheduler.add_noise(z0, noise, timesteps[:1])``; with a mask at strength 1.0 as ``noise * init_noise_sigma``.
The GM branch has no picture to start from, and a gain map started part-way down the schedule from pure noise is outside what the GM
UNet was trained on.  So the GM scheduler (the deep copy taken before ``set_begin_index``) always runs the WHOLE schedule from
``noise * init_noise_sigma``: for the first ``t_start * order`` iterations the GM UNet runs alone with ``z0`` as its SDR operand --
what ``StableDiffusionGMPipeline`` feeds it for a photograph -- and from then on the loop is the joint loop above.  Per iteration a
shared generator is consumed by the GM scheduler alone at first, SDR before GM afterwards.
Mask, after every SDR step i (diffusers' inpaint rule): ``keep = add_noise(z0, noise, timesteps[i + 1])`` (``z0`` at the last step),
``latents = (1 - m) * keep + m * latents``; and the x0 handed to the GM UNet is ``(1 - m) * z0 + m * x0``: where the picture is kept
it is known, so the gain map sees it.  The schedulers' multistep history is not blended (nor is it in diffusers).  Fused path: ONE
launch per step (gmd_inpaint_blend, in place on the step's two outputs, on the SDR stream before the GM stream waits for x0); mask,
z0 and noise are written once, outside any graph.  The generic loop does the same in torch expressions.  Refused by name: a mask with
an SDR UNet of ``in_channels == 9`` (inpainting checkpoints), ``padding_mask_crop``, ``masked_image_latents``.
"""
from __future__ import annotations

import copy
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from .. import hip_ops as ops
from .stable_diffusion_gm import _GMPipelineBase, _per_call_lora_scale, rescale_noise_cfg, retrieve_timesteps

__all__ = ["StableDiffusionDualUNetPipeline", "rescale_noise_cfg", "retrieve_timesteps"]


class StableDiffusionDualUNetPipeline(_GMPipelineBase):
    # Run the GM UNet on a second HIP stream, one step behind the SDR UNet (GM(i) needs only x0_i, SDR(i+1) only
    # latents_{i+1}).  Measured on MI355X (bench.py): eager launches 3.04 vs 3.04 images/s (the host, ~10 us per launch,
    # cannot keep two streams fed); with each forward replayed from a captured HIP graph 3.04 -> 3.86 images/s.
    overlap_streams = True
    # Launch-plan family of the two UNet forwards (hip_ops.plan_family): None = by regime -- the co-running family when the forwards
    # overlap on two streams, the launch-by-launch plans when they share one stream; True / False pin it (bench.py pins True for
    # its instrumented single-stream step so that it times, and compares bit for bit, the kernels the shipped path runs)
    co_run_plans = None
    _step_probe = None  # test hook: callable(i, sdr_latents, gm_latents) after every loop iteration

    _optional_components = ["safety_checker", "feature_extractor", "image_encoder", "controlnet"]

    def __init__(self, vae, text_encoder, tokenizer, unet, gm_unet, scheduler, safety_checker, feature_extractor,
                 image_encoder=None, requires_safety_checker: bool = True, controlnet=None):
        if isinstance(controlnet, (list, tuple)):
            raise NotImplementedError("a list of ControlNets (diffusers' MultiControlNetModel) is not implemented: pass one ControlNetModel")
        self._init_common(vae, text_encoder, tokenizer, unet, scheduler, safety_checker, feature_extractor, image_encoder,
                          requires_safety_checker, gm_unet=gm_unet, controlnet=controlnet)

    # ---- ControlNet conditioning of the SDR UNet (the GM UNet follows the SDR x0 and is never conditioned) -------------------------
    def _prepare_control_image(self, image, height, width, rows, device):
        """diffusers' control-image preparation as far as it applies here: float32 NCHW in [0, 1] (no normalisation) of exactly
        ``height`` x ``width``, one image per latent row (a single image serves every row).  Tensors [B, 3, H, W] / [3, H, W] in
        [0, 1], uint8 arrays [H, W, 3] / [B, H, W, 3] and PIL images are taken; a wrong size is an error, not a resize."""
        if image is None:
            raise ValueError("this pipeline has a controlnet: `control_image` is required")
        if isinstance(image, (list, tuple)):
            if len(image) == 0:
                raise ValueError("`control_image` is an empty list")
            image = [self._prepare_control_image(im, height, width, 1, "cpu") for im in image]
            image = torch.cat(image, 0)
        elif not torch.is_tensor(image):
            import numpy as np

            arr = np.asarray(image)
            if arr.ndim == 2:
                arr = np.stack([arr] * 3, -1)
            if arr.ndim == 3:
                arr = arr[None]
            if arr.ndim != 4 or arr.shape[-1] != 3:
                raise ValueError(f"`control_image` must be an RGB image; got an array of shape {arr.shape}")
            t = torch.from_numpy(np.ascontiguousarray(arr)).permute(0, 3, 1, 2)
            image = t.float() / 255.0 if t.dtype == torch.uint8 else t.float()
        if image.dim() == 3:
            image = image[None]
        if image.dim() != 4 or tuple(image.shape[-2:]) != (height, width):
            raise ValueError(f"`control_image` must be {height} x {width} (height x width of this call); got {tuple(image.shape)}")
        if image.shape[0] == 1 and rows > 1:
            image = image.expand(rows, -1, -1, -1)
        if image.shape[0] != rows:
            raise ValueError(f"`control_image` holds {image.shape[0]} images for {rows} latents")
        return image.to(device=device, dtype=torch.float32).contiguous()

    # ---- IP-Adapter image prompting of the SDR UNet (stable_diffusion_dual_unet.py:518-585, 986-1020) -----------------------------
    _ip_adapter_supported = True

    def load_ip_adapter(self, path_or_state_dict, subfolder=None, weight_name=None):
        """diffusers' ``load_ip_adapter`` for LOCAL files: a ``.safetensors`` file whose keys carry the ``image_proj.`` / ``ip_adapter.``
        prefixes, a ``.bin`` torch pickle of the two dicts (read with ``weights_only=True``), or the already-loaded dict
        ``{"image_proj": ..., "ip_adapter": ...}``.  ``path_or_state_dict`` may be the file itself or a directory joined with
        ``subfolder`` and ``weight_name``.  The adapter goes into the SDR UNet (``pipe.gm_unet.load_ip_adapter`` prompts the GM UNet as
        well); the image encoder is the constructor's ``image_encoder`` and is never loaded from the adapter's folder."""
        import os

        sd = path_or_state_dict
        if not isinstance(sd, dict):
            path = os.fspath(sd)
            if os.path.isdir(path):
                if weight_name is None:
                    raise ValueError("load_ip_adapter: `weight_name` is required when a directory is given")
                path = os.path.join(path, subfolder or "", weight_name)
            if not os.path.isfile(path):
                raise FileNotFoundError(f"load_ip_adapter: {path} is not a local file (nothing is downloaded)")
            if path.endswith(".safetensors"):
                from safetensors import safe_open

                sd = {"image_proj": {}, "ip_adapter": {}}
                with safe_open(path, framework="pt", device="cpu") as f:
                    for key in f.keys():
                        if key.startswith("image_proj."):
                            sd["image_proj"][key[len("image_proj."):]] = f.get_tensor(key)
                        elif key.startswith("ip_adapter."):
                            sd["ip_adapter"][key[len("ip_adapter."):]] = f.get_tensor(key)
            else:
                sd = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(sd, dict) or sorted(sd.keys()) != ["image_proj", "ip_adapter"]:
            raise ValueError("Required keys are (`image_proj` and `ip_adapter`) missing from the state dict.")
        self.unet.load_ip_adapter(sd)

    def unload_ip_adapter(self):
        self.unet.unload_ip_adapter()

    def set_ip_adapter_scale(self, scale):
        self.unet.set_ip_adapter_scale(scale)

    def encode_image(self, image, device, num_images_per_prompt, output_hidden_states=None):
        """stable_diffusion_dual_unet.py:518-540.  ``image_encoder`` / ``feature_extractor`` are whatever the constructor got
        (``image_encoder(pixels).image_embeds``; transformers' CLIPVisionModelWithProjection works); they run in torch, once per call."""
        if output_hidden_states:
            raise NotImplementedError("IP-Adapter Plus (hidden states of the image encoder through a Resampler) is not implemented")
        if getattr(self, "image_encoder", None) is None:
            raise ValueError("`ip_adapter_image` needs an `image_encoder` (constructor argument); pass `ip_adapter_image_embeds` instead")
        params = getattr(self.image_encoder, "parameters", None)
        first = next(iter(params()), None) if callable(params) else None
        dtype = first.dtype if first is not None else torch.float32
        if not isinstance(image, torch.Tensor):
            if getattr(self, "feature_extractor", None) is None:
                raise ValueError("`ip_adapter_image` that is not a tensor of pixel values needs a `feature_extractor`")
            image = self.feature_extractor(image, return_tensors="pt").pixel_values
        image = image.to(device=device, dtype=dtype)
        image_embeds = self.image_encoder(image).image_embeds
        image_embeds = image_embeds.repeat_interleave(num_images_per_prompt, dim=0)
        uncond_image_embeds = torch.zeros_like(image_embeds)
        return image_embeds, uncond_image_embeds

    def prepare_ip_adapter_image_embeds(self, ip_adapter_image, ip_adapter_image_embeds, device, num_images_per_prompt,
                                        do_classifier_free_guidance):
        """stable_diffusion_dual_unet.py:542-585: a list with one tensor per adapter, [negative; positive] rows under guidance (zeros
        are the negative image embedding; given embeddings carry their own negative half and are ``chunk(2)``-ed)."""
        image_embeds = []
        if do_classifier_free_guidance:
            negative_image_embeds = []
        n_adapters = 1 if self.unet.has_ip_adapter else 0
        if ip_adapter_image_embeds is None:
            if not isinstance(ip_adapter_image, list):
                ip_adapter_image = [ip_adapter_image]
            if len(ip_adapter_image) != n_adapters:
                raise ValueError(f"`ip_adapter_image` must have same length as the number of IP Adapters. Got {len(ip_adapter_image)} "
                                 f"images and {n_adapters} IP Adapters.")
            for single_ip_adapter_image in ip_adapter_image:
                single_image_embeds, single_negative_image_embeds = self.encode_image(single_ip_adapter_image, device, 1, False)
                image_embeds.append(single_image_embeds[None, :])
                if do_classifier_free_guidance:
                    negative_image_embeds.append(single_negative_image_embeds[None, :])
        else:
            for single_image_embeds in ip_adapter_image_embeds:
                if do_classifier_free_guidance:
                    single_negative_image_embeds, single_image_embeds = single_image_embeds.chunk(2)
                    negative_image_embeds.append(single_negative_image_embeds)
                image_embeds.append(single_image_embeds)
        ip_adapter_image_embeds = []
        for i, single_image_embeds in enumerate(image_embeds):
            single_image_embeds = torch.cat([single_image_embeds] * num_images_per_prompt, dim=0)
            if do_classifier_free_guidance:
                single_negative_image_embeds = torch.cat([negative_image_embeds[i]] * num_images_per_prompt, dim=0)
                single_image_embeds = torch.cat([single_negative_image_embeds, single_image_embeds], dim=0)
            single_image_embeds = single_image_embeds.to(device=device)
            ip_adapter_image_embeds.append(single_image_embeds)
        return ip_adapter_image_embeds

    def _image_prompt_rows(self, ip_adapter_image, ip_adapter_image_embeds, device, rows, do_cfg):
        """The one adapter's image embeddings [(2 if do_cfg else 1) * rows, n_images, clip_dim], or None without an image prompt.
        No broadcasting: a row count other than the latents' (doubled under guidance) is an error, as in diffusers."""
        if ip_adapter_image is None and ip_adapter_image_embeds is None:
            return None
        if not self.unet.has_ip_adapter:
            raise ValueError("an image prompt was given but no IP-Adapter is loaded: call load_ip_adapter() first")
        embeds = self.prepare_ip_adapter_image_embeds(ip_adapter_image, ip_adapter_image_embeds, device, rows, do_cfg)
        if len(embeds) != 1:
            raise NotImplementedError(f"{len(embeds)} image-embedding tensors: several IP-Adapters at once are not implemented")
        e = embeds[0]
        if e.dim() == 4:
            raise NotImplementedError("4-D image embeddings (hidden states for IP-Adapter Plus) are not implemented")
        want = (2 if do_cfg else 1) * rows
        if e.dim() != 3 or e.shape[0] != want:
            raise ValueError(f"the image prompt has {e.shape[0]} rows for {want} UNet rows (batch x num_images_per_prompt"
                             f"{', doubled under guidance' if do_cfg else ''}); given embeddings are repeated, never broadcast")
        return e

    @staticmethod
    def _control_keep(n, start, end):
        from ..components.controlnet import control_window

        return [control_window(i, n, start, end) for i in range(n)]

    @staticmethod
    def _batched_added_cond(added_cond, do_cfg, device):
        """(SDR UNet's, GM UNet's) added_cond_kwargs: [negative; positive] rows for the guidance batch, the positive rows for the
        GM UNet (it runs the conditional half only, like its prompt embeddings); (None, None) without added conditioning."""
        if not added_cond:
            return None, None
        pos = {k: added_cond[k].to(device) for k in ("text_embeds", "time_ids")}
        if not do_cfg:
            return pos, pos
        if "negative_text_embeds" not in added_cond:
            raise ValueError("classifier-free guidance with an SDXL-style UNet needs added_cond_kwargs['negative_text_embeds']")
        neg_ids = added_cond.get("negative_time_ids", added_cond["time_ids"]).to(device)
        return dict(text_embeds=torch.cat([added_cond["negative_text_embeds"].to(device), pos["text_embeds"]]),
                    time_ids=torch.cat([neg_ids, pos["time_ids"]])), pos

    # ---- img2img / inpainting (see the module docstring) ---------------------------------------------------------------------------
    def _encode_init_image(self, image, height, width, rows, shape, dtype, device, generator):
        """``z0`` [rows, 4, h, w] of ``dtype`` on ``device``: the clean latents of ``image``, already multiplied by
        ``scaling_factor``.  A tensor with 4 channels is taken as such latents (diffusers); anything else goes through
        ``VaeImageProcessor.preprocess`` and ``vae.encode(x).latent_dist.sample(generator)``: the call's first draw."""
        if torch.is_tensor(image) and image.dim() == 4 and image.shape[1] == 4:
            z0 = image.to(device=device, dtype=dtype)
        else:
            from ..components.autoencoder_kl import AutoencoderKL

            if isinstance(self.vae, AutoencoderKL) and ops.is_half(self.vae.dtype):
                raise ValueError(f"`image` as pixels needs a float32 AutoencoderKL (this one is {self.vae.dtype}: its encoder's 8-channel"
                                 " quant_conv is no 16-bit matrix-core shape); encode the picture with a float32 copy and pass the latents"
                                 " (`vae.encode(x).latent_dist.sample(generator) * vae.config.scaling_factor`) as `image`")
            x = self.image_processor.preprocess(image, height, width).to(device)
            if isinstance(generator, list) and x.shape[0] == 1 and rows > 1:
                x = x.expand(rows, -1, -1, -1).contiguous()  # one draw per generator
            z0 = self.vae.encode(x).latent_dist.sample(generator).to(dtype) * self.vae.config.scaling_factor
        if z0.shape[0] == 1 and rows > 1:
            z0 = z0.expand(rows, -1, -1, -1)
        if tuple(z0.shape) != tuple(shape):
            raise ValueError(f"`image` gives latents of shape {tuple(z0.shape)} for this call's {tuple(shape)} (rows = batch x "
                             "num_images_per_prompt; one image is repeated)")
        return z0.contiguous()

    @staticmethod
    def _prepare_inpaint_mask(mask, height, width, h, w, rows, device):
        """float32 [1 | rows, 1, h, w], 1 = repaint, 0 = keep.  An image-size mask ([H, W] or [1 | rows, 1, H, W]: float, uint8 with
        255 = 1, PIL "L") is binarised at 0.5 and brought to latent size with ``F.interpolate`` (nearest), as diffusers'
        ``prepare_mask_latents`` does; a float mask that already has the latent size is taken as it is."""
        if not torch.is_tensor(mask):
            import numpy as np

            mask = torch.from_numpy(np.ascontiguousarray(np.array(mask)))  # (a copy: a PIL image's buffer is read-only)
        if mask.dtype == torch.uint8:
            mask = mask.to(torch.float32) / 255.0
        elif mask.dtype == torch.bool:
            mask = mask.to(torch.float32)
        elif not mask.is_floating_point():
            raise ValueError(f"`mask_image` must be float, uint8 or bool (got {mask.dtype})")
        mask = mask.to(torch.float32)
        if mask.dim() == 2:
            mask = mask[None, None]
        if mask.dim() != 4 or mask.shape[1] != 1 or mask.shape[0] not in (1, rows):
            raise ValueError(f"`mask_image` must be [H, W] or [1 | {rows}, 1, H, W] (got {tuple(mask.shape)})")
        if tuple(mask.shape[-2:]) != (h, w):
            if tuple(mask.shape[-2:]) != (height, width):
                raise ValueError(f"`mask_image` must be {height} x {width} (this call) or {h} x {w} (its latents); got"
                                 f" {mask.shape[-2]} x {mask.shape[-1]}")
            mask = (mask >= 0.5).to(torch.float32)
            mask = torch.nn.functional.interpolate(mask, size=(h, w))
        return mask.to(device).contiguous()

    def _gm_stream(self, device):
        return ops.side_stream(device)  # one per device for the whole process, not per pipeline object (see there)

    @_per_call_lora_scale
    @torch.no_grad()
    def __call__(
        self,
        prompt: Union[str, List[str]] = None,
        height: Optional[int] = None,
        width: Optional[int] = None,
        num_inference_steps: int = 50,
        timesteps: List[int] = None,
        sigmas: List[float] = None,
        guidance_scale: float = 7.5,
        negative_prompt: Optional[Union[str, List[str]]] = None,
        num_images_per_prompt: Optional[int] = 1,
        eta: float = 0.0,
        generator: Optional[Union[torch.Generator, List[torch.Generator]]] = None,
        latents: Optional[torch.Tensor] = None,
        prompt_embeds: Optional[torch.Tensor] = None,
        negative_prompt_embeds: Optional[torch.Tensor] = None,
        ip_adapter_image=None,
        ip_adapter_image_embeds: Optional[List[torch.Tensor]] = None,
        output_type: Optional[str] = "pil",
        return_dict: bool = True,
        cross_attention_kwargs: Optional[Dict[str, Any]] = None,
        guidance_rescale: float = 0.0,
        clip_skip: Optional[int] = None,
        callback_on_step_end: Optional[Callable[[Any, int, Any, Dict], Dict]] = None,
        callback_on_step_end_tensor_inputs: List[str] = ["latents"],
        **kwargs,
    ):
        callback, callback_steps = self._pop_legacy_callbacks(kwargs)
        # EXTENSION beyond the reference (which has no SDXL path: its added_cond_kwargs carry IP-adapter image embeddings only,
        # stable_diffusion_gm.py:1022-1026): for UNets with addition_embed_type "text_time" the caller passes
        # added_cond_kwargs = {"text_embeds", "time_ids"[, "negative_text_embeds", "negative_time_ids"]}; every other unknown
        # keyword is ignored as in the reference
        added_cond = kwargs.pop("added_cond_kwargs", None)
        # img2img / inpainting (module docstring): diffusers' keywords, read here and given meaning only when `image` is there
        image, strength, mask_image = kwargs.pop("image", None), kwargs.pop("strength", None), kwargs.pop("mask_image", None)
        for refused in ("padding_mask_crop", "masked_image_latents"):
            if kwargs.pop(refused, None) is not None:
                raise NotImplementedError(f"`{refused}` is not implemented: the inpainting of this pipeline keeps a region of the"
                                          " latents of a 4-channel SDR UNet (`image`, `mask_image`, `strength`)")
        if image is None and (mask_image is not None or strength is not None):
            raise ValueError("`mask_image` and `strength` belong to img2img / inpainting: they need `image`")
        if image is not None:
            if mask_image is not None and self.unet.config.in_channels != 4:
                raise NotImplementedError(f"`mask_image` with an SDR UNet of in_channels == {self.unet.config.in_channels} is not implemented"
                                          " (9-channel inpainting checkpoints take the mask and the masked image as UNet input):"
                                          " the mask keeps a region of the latents of a 4-channel UNet")
            strength = float(strength) if strength is not None else (0.8 if mask_image is None else 1.0)
            if not 0.0 <= strength <= 1.0:
                raise ValueError(f"The value of strength should in [0.0, 1.0] but is {strength}")
        if hasattr(callback_on_step_end, "tensor_inputs"):
            callback_on_step_end_tensor_inputs = callback_on_step_end.tensor_inputs
        height, width = self._default_hw(height, width)
        self.check_inputs(prompt, height, width, callback_steps, negative_prompt, prompt_embeds, negative_prompt_embeds,
                          ip_adapter_image, ip_adapter_image_embeds, callback_on_step_end_tensor_inputs)
        self._guidance_scale = guidance_scale
        self._guidance_rescale = guidance_rescale
        self._clip_skip = clip_skip
        self._cross_attention_kwargs = cross_attention_kwargs
        self._interrupt = False

        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]
        device = self._execution_device
        # ControlNet conditioning of the SDR UNet (diffusers' StableDiffusionControlNetPipeline keywords).  Without a controlnet the
        # five keywords stay in **kwargs and are ignored, as every unknown keyword is.
        cn = getattr(self, "controlnet", None)
        if cn is not None:
            cn_scale = kwargs.pop("controlnet_conditioning_scale", 1.0)
            guess_mode = bool(kwargs.pop("guess_mode", False))
            cg_start, cg_end = kwargs.pop("control_guidance_start", 0.0), kwargs.pop("control_guidance_end", 1.0)
            if any(isinstance(v, (list, tuple)) for v in (cn_scale, cg_start, cg_end)):
                raise NotImplementedError("per-ControlNet lists of scales / guidance windows belong to Multi-ControlNet, which is not implemented")
            cn_scale, cg_start, cg_end = float(cn_scale), float(cg_start), float(cg_end)
            if cg_start >= cg_end or cg_start < 0.0 or cg_end > 1.0:
                raise ValueError(f"control guidance window [{cg_start}, {cg_end}] must satisfy 0 <= start < end <= 1")
            control_image = self._prepare_control_image(kwargs.pop("control_image", None), height, width,
                                                        batch_size * num_images_per_prompt, "cpu")
        lora_scale = self.cross_attention_kwargs.get("scale", None) if self.cross_attention_kwargs is not None else None
        self._apply_lora_scale(lora_scale)
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, device, num_images_per_prompt, self.do_classifier_free_guidance, negative_prompt,
            prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, lora_scale=lora_scale,
            clip_skip=self.clip_skip)
        do_cfg = self.do_classifier_free_guidance
        n_neg = negative_prompt_embeds.shape[0] if do_cfg else 0
        if do_cfg:
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds])
        gm_prompt_embeds = prompt_embeds[n_neg:]  # conditional half (vis.py:274)
        # dual.py:986-993: the image prompt, [negative; positive] rows like the text.  Only the SDR UNet is image-prompted, unless an
        # adapter was loaded into the GM UNet itself: it then gets the positive rows, like its prompt embeddings
        image_rows = self._image_prompt_rows(ip_adapter_image, ip_adapter_image_embeds, device, batch_size * num_images_per_prompt, do_cfg)
        gm_image_rows = None
        if image_rows is not None and self.gm_unet.has_ip_adapter:
            gm_image_rows = image_rows[image_rows.shape[0] // 2:] if do_cfg else image_rows

        sdr_from = 0  # the iteration the SDR branch enters the loop at: 0 without `image`
        if image is None:
            timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device, timesteps, sigmas)
        else:
            from ..components.schedulers import LCMScheduler

            if num_inference_steps is not None and int(num_inference_steps * strength) < 1:
                raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of pipeline"
                                 f" steps is {int(num_inference_steps * strength)} which is < 1 and not appropriate for this pipeline.")
            if isinstance(self.scheduler, LCMScheduler):  # the LCM schedule is built for the strength: nothing to slice
                timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device, timesteps, sigmas,
                                                                    strength=strength)
            else:
                timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device, timesteps, sigmas)
                init_timestep = min(int(num_inference_steps * strength), num_inference_steps)  # diffusers' get_timesteps
                if init_timestep < 1:
                    raise ValueError(f"After adjusting the num_inference_steps by strength parameter: {strength}, the number of"
                                     f" pipeline steps is {init_timestep} which is < 1 and not appropriate for this pipeline.")
                sdr_from = max(num_inference_steps - init_timestep, 0) * self.scheduler.order

        num_channels_latents = self.unet.config.in_channels
        z0 = noise = inpaint_mask = None
        if image is None:
            latents = self.prepare_latents(batch_size * num_images_per_prompt, num_channels_latents, height, width,
                                           self._latent_dtype(prompt_embeds, device), device, generator, latents)
            gm_latents = latents.clone()  # dual.py:1012: both streams start from the same (scaled) noise
        else:
            from ..components.image_processor import randn_tensor

            n_rows, lat_dtype = batch_size * num_images_per_prompt, self._latent_dtype(prompt_embeds, device)
            shape = (n_rows, num_channels_latents, int(height) // self.vae_scale_factor, int(width) // self.vae_scale_factor)
            if isinstance(generator, list) and len(generator) != n_rows:
                raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                                 f" size of {n_rows}. Make sure the batch size matches the length of the generators.")
            # generator order: the encoder's sample (pixels only), the noise, then the steps' own draws
            z0 = self._encode_init_image(image, height, width, n_rows, shape, lat_dtype, device, generator)
            noise = (randn_tensor(shape, generator=generator, device=device, dtype=lat_dtype) if latents is None
                     else latents.to(device)).contiguous()
            if mask_image is not None:
                inpaint_mask = self._prepare_inpaint_mask(mask_image, height, width, shape[2], shape[3], n_rows, z0.device).to(lat_dtype)
            # the GM branch has no picture to start from: it runs the whole schedule from the noise.  The SDR start needs the begin
            # index, which is set below, after the GM scheduler was copied: until then `latents` stands for its shape and dtype
            gm_latents = noise * self.scheduler.init_noise_sigma
            latents = gm_latents
        extra_step_kwargs = self.prepare_extra_step_kwargs(generator, eta)
        # dual.py:1024-1030: the guidance-scale embedding of a guidance-embedded (LCM) UNet, each UNet at its own width (see the module
        # docstring); do_classifier_free_guidance is False for such an SDR UNet
        rows = batch_size * num_images_per_prompt
        timestep_cond = self._timestep_cond_for(self.unet, rows, device, latents.dtype)
        gm_timestep_cond = self._timestep_cond_for(self.gm_unet, rows, device, latents.dtype)

        num_warmup_steps = len(timesteps) - num_inference_steps * self.scheduler.order
        self._num_timesteps = len(timesteps)
        self.gm_scheduler = copy.deepcopy(self.scheduler)  # dual.py:1037, after set_timesteps

        sdr_added, gm_added = self._batched_added_cond(added_cond, do_cfg, latents.device)
        ip_ctx = gm_ip_ctx = None
        fused = self._use_fused(latents, self.unet, self.scheduler) and self._use_fused(latents, self.gm_unet, self.gm_scheduler)
        if image is not None:
            # the SDR branch enters the schedule at `sdr_from` (the GM scheduler, copied above, runs all of it)
            if hasattr(self.scheduler, "set_begin_index") and not isinstance(self.scheduler, LCMScheduler):
                self.scheduler.set_begin_index(sdr_from)
            if inpaint_mask is not None and strength == 1.0:  # diffusers' is_strength_max: pure noise, the picture only where kept
                latents = noise * self.scheduler.init_noise_sigma
            elif fused:
                latents = ops.inpaint_blend(z0, x_prev=torch.empty_like(z0), noise=noise,
                                            coefs=self.scheduler.add_noise_coefs(timesteps[sdr_from]))[0]
            else:
                latents = self.scheduler.add_noise(z0, noise, timesteps[sdr_from:sdr_from + 1])
        keep = None  # per step: does the ControlNet run (diffusers' control guidance window); None without a controlnet
        if cn is not None:
            keep = self._control_keep(len(timesteps) - sdr_from, cg_start, cg_end)  # over the SDR branch's steps: keep[i - sdr_from]
            cn_half = guess_mode and do_cfg  # guess mode: the ControlNet sees the conditional half only
            control_image = control_image.to(latents.device)
            if do_cfg and not cn_half:
                control_image = torch.cat([control_image] * 2)
            cn_embeds = prompt_embeds[n_neg:] if cn_half else prompt_embeds
            if fused and (cn.dtype != self.unet.dtype or cn.device != self.unet.device):
                raise ValueError(f"the controlnet ({cn.dtype} on {cn.device}) must share the SDR UNet's dtype and device "
                                 f"({self.unet.dtype} on {self.unet.device}): its residuals are added in the UNet's own kernels")
        if fused:
            ctx = self.unet.prepare_context(prompt_embeds)
            gm_ctx = self.gm_unet.prepare_context(gm_prompt_embeds)
            h, w = latents.shape[-2:]
            # constant over the loop: written once into the persistent buffers the (captured) forwards read
            self.unet.set_added_cond(sdr_added, (2 if do_cfg else 1) * latents.shape[0])
            self.gm_unet.set_added_cond(gm_added, latents.shape[0])
            self.unet.set_timestep_cond(timestep_cond, (2 if do_cfg else 1) * latents.shape[0])
            self.gm_unet.set_timestep_cond(gm_timestep_cond, latents.shape[0])
            # the image prompt: projected and turned into every layer's K_ip / V_ip^T once, outside any graph
            if image_rows is not None:
                ip_ctx = self.unet.prepare_ip_context(image_rows.to(latents.device))
            if gm_image_rows is not None:
                gm_ip_ctx = self.gm_unet.prepare_ip_context(gm_image_rows.to(latents.device))
            # The GM UNet of step i needs only x0_i; the SDR UNet of step i+1 needs only latents_{i+1}: the two are
            # independent, so the GM stream runs on its own HIP stream one step behind the SDR stream and their
            # kernels overlap (the batch-B GM kernels alone cannot fill 256 CUs).
            sdr_stream = torch.cuda.current_stream(latents.device)
            gm_stream = self._gm_stream(latents.device) if self.overlap_streams else sdr_stream
            ts_host = timesteps.tolist()  # host copy: no device sync inside the loop (ints, or a sigma-space scheduler's floats)
            ts_dev = timesteps.to(device=latents.device, dtype=torch.float32)
            g_sdr = g_gm = None
            shared = self._cfg_shared(self.unet, do_cfg)
            nb_sdr = (2 if do_cfg else 1) * latents.shape[0]
            # two forwards in flight side by side: their contractions take the co-running plan family (fewest L2 -> LDS bytes per
            # product; -2.2 % per batch against the launch-by-launch plans, +8.6 % if the streams were serialised:
            # profiles/r05_ab_plan_default.txt), a single-stream run keeps the plans that are fastest alone
            co_run = (gm_stream is not sdr_stream) if self.co_run_plans is None else bool(self.co_run_plans)
            g_cn = g_sdr_c = control = None
            if cn is not None:
                # constant over the loop, written once outside any graph: the conditioning embedding and the thirteen scales.  The
                # ControlNet runs on the SDR stream in front of the UNet that reads its residuals; it has no CFG shared prefix, so it
                # takes the duplicated batch (or, in guess mode, the conditional half: the UNet then skips the unconditional samples)
                cn_rows = latents.shape[0] if cn_half else nb_sdr
                cn_ctx = cn.prepare_context(cn_embeds)
                cn.set_condition(control_image, cn_rows)
                cn_scales = cn.set_scales(cn_scale, guess_mode)
                cn_skip = nb_sdr - cn_rows
            if self._graphs_ok():
                if cn is None or not all(keep):
                    g_sdr = self.unet.graphed_forward(nb_sdr, h, w, ctx, cfg_shared=shared, co_run=co_run, ip=ip_ctx)
                if cn is not None and any(keep):
                    g_cn = cn.graphed_forward(cn_rows, h, w, cn_ctx, co_run=co_run)
                    control = (g_cn.down, g_cn.mid, cn_scales, cn_skip)
                    g_sdr_c = self.unet.graphed_forward(nb_sdr, h, w, ctx, cfg_shared=shared, co_run=co_run, control=control, ip=ip_ctx)
                g_gm = self.gm_unet.graphed_forward(latents.shape[0], h, w, gm_ctx, co_run=co_run, ip=gm_ip_ctx)
            pre = self._predraw_step_noise([self.scheduler, self.gm_scheduler], ts_host, latents.shape, generator, latents.device,
                                           eta=extra_step_kwargs.get("eta", 0.0), **({"first": (sdr_from, 0)} if sdr_from else {}))
            gm_stream.wait_stream(sdr_stream)
            if gm_stream is not sdr_stream:
                # allocated on the caller's stream, consumed (and released) by step 0 on the GM stream: without this the
                # allocator may hand the block to the SDR stream's step 1 while GM step 0 still reads it
                gm_latents.record_stream(gm_stream)
                if sdr_from:
                    z0.record_stream(gm_stream)  # the GM UNet's SDR operand while the SDR branch waits
        elif image_rows is not None:
            # dual.py:1017-1022, 1058: added_cond_kwargs = {"image_embeds": [...]}, diffusers' list with one tensor per adapter
            sdr_added = {**(sdr_added or {}), "image_embeds": [image_rows.to(latents.device)]}
            if gm_image_rows is not None:
                gm_added = {**(gm_added or {}), "image_embeds": [gm_image_rows.to(latents.device)]}
        if not fused and getattr(self.scheduler, "sigma_space", False):
            raise ValueError(
                f"{type(self.scheduler).__name__} is a sigma-space scheduler; the dual-UNet pipeline runs it on the fused device path only"
                " (float32 latents on the GPU with the HIP UNets).  The generic loop restates the reference, which indexes"
                " alphas_cumprod with the (fractional) timestep and overwrites the GM latents with their scaled copy.")

        with self.progress_bar(total=num_inference_steps) as progress_bar:
            for i, t in enumerate(timesteps):
                if self.interrupt:
                    continue
                if fused:
                    if i >= sdr_from:  # (img2img: the GM branch runs alone until the SDR branch enters the schedule)
                        div = self._pack_div(self.scheduler, ts_host[i])
                        use_cn = cn is not None and keep[i - sdr_from]  # inside the control guidance window: ControlNet, then the UNet's control graph
                        g_step = g_sdr_c if use_cn else g_sdr
                        x = self.unet.pack_input(latents, dup=2 if (do_cfg and not shared) else 1, out=g_step.x if g_step else None,
                                                 **({"div": (div, 1.0)} if div is not None else {}))
                        self.unet.set_timestep_from(ts_dev, i)
                        if use_cn:  # the same latents and timestep, packed for the ControlNet's own batch
                            cx = cn.pack_input(latents, dup=2 if (do_cfg and not cn_half) else 1, out=g_cn.x if g_cn else None,
                                               **({"div": (div, 1.0)} if div is not None else {}))
                            cn.set_timestep_from(ts_dev, i)
                        if g_step:
                            if use_cn:
                                g_cn.replay()
                            sdr_noise_pred = g_step.replay()
                        elif use_cn:
                            with ops.plan_family(co_run):
                                c_down, c_mid = cn.forward_packed(cx, cn_rows, h, w, cn_ctx)
                                sdr_noise_pred = self.unet.forward_packed(x, nb_sdr, h, w, ctx, cfg_shared=shared, ip=ip_ctx,
                                                                          control=(c_down, c_mid, cn_scales, cn_skip))
                        else:
                            with ops.plan_family(co_run):
                                sdr_noise_pred = self.unet.forward_packed(x, nb_sdr, h, w, ctx, cfg_shared=shared, ip=ip_ctx)
                        pre_step = latents
                        latents, x0_latent = self.scheduler.fused_step(sdr_noise_pred, ts_host[i], pre_step, do_cfg, self.guidance_scale,
                                                                       self.guidance_rescale if do_cfg else 0.0, want_x0=True,
                                                                       **self._fused_step_kwargs(extra_step_kwargs),
                                                                       **({"noise": pre[0][i]} if pre else {}))
                        if inpaint_mask is not None:
                            # diffusers' inpaint rule and the x0 the GM UNet sees, one launch on the SDR stream, in place on the
                            # step's own outputs: the kept region returns to the picture at the next step's noise level
                            last = i == len(ts_host) - 1
                            ops.inpaint_blend(z0, x_prev=latents, x0=x0_latent, mask=inpaint_mask, noise=None if last else noise,
                                              coefs=(1.0, 0.0) if last else self.scheduler.add_noise_coefs(ts_host[i + 1]))
                    with torch.cuda.stream(gm_stream):
                        if i >= sdr_from:
                            gm_stream.wait_stream(sdr_stream)  # x0_i is ready
                            x0_latent.record_stream(gm_stream)
                        else:
                            x0_latent = z0  # what StableDiffusionGMPipeline feeds the GM UNet: a picture's own latents
                        gm_div = self._pack_div(self.gm_scheduler, ts_host[i])  # x0 is a clean-image estimate: never scaled
                        gx = self.gm_unet.pack_input((x0_latent, gm_latents), dup=1, out=g_gm.x if g_gm else None,
                                                     **({"div": (1.0, gm_div)} if gm_div is not None else {}))
                        self.gm_unet.set_timestep_from(ts_dev, i)
                        if g_gm:
                            gm_noise_pred = g_gm.replay()
                        else:
                            with ops.plan_family(co_run):
                                gm_noise_pred = self.gm_unet.forward_packed(gx, gx.shape[0], h, w, gm_ctx, ip=gm_ip_ctx)
                        gm_latents = self.gm_scheduler.step(gm_noise_pred, ts_host[i], gm_latents,
                                                            **self._fused_step_kwargs(extra_step_kwargs),
                                                            **({"noise": pre[1][i]} if pre else {}), return_dict=False)[0]
                elif i < sdr_from:
                    # img2img: the GM branch alone, on the picture's own latents, until the SDR branch enters the schedule
                    gm_latents = self.gm_scheduler.scale_model_input(gm_latents, t)
                    gm_latent_input = torch.cat([z0, gm_latents], dim=1)
                    gm_noise_pred = self.gm_unet(gm_latent_input, t, encoder_hidden_states=gm_prompt_embeds, timestep_cond=gm_timestep_cond,
                                                 cross_attention_kwargs=self.cross_attention_kwargs, added_cond_kwargs=gm_added,
                                                 return_dict=False)[0]
                    gm_latents = self.gm_scheduler.step(gm_noise_pred, t, gm_latents, **extra_step_kwargs, return_dict=False)[0]
                else:
                    latent_model_input = torch.cat([latents] * 2) if do_cfg else latents
                    latent_model_input = self.scheduler.scale_model_input(latent_model_input, t)
                    gm_latents = self.gm_scheduler.scale_model_input(gm_latents, t)
                    cn_kw = {}
                    if cn is not None and keep[i - sdr_from]:
                        # diffusers' StableDiffusionControlNetPipeline: guess mode infers the conditional half only and pads the
                        # unconditional half's residuals with zeros
                        c_in = self.scheduler.scale_model_input(latents, t) if cn_half else latent_model_input
                        c_down, c_mid = cn(c_in, t, cn_embeds, controlnet_cond=control_image, conditioning_scale=cn_scale,
                                           guess_mode=guess_mode, return_dict=False)
                        if cn_half:
                            c_down = [torch.cat([torch.zeros_like(d), d]) for d in c_down]
                            c_mid = torch.cat([torch.zeros_like(c_mid), c_mid])
                        cn_kw = dict(down_block_additional_residuals=c_down, mid_block_additional_residual=c_mid)
                    sdr_noise_pred = self.unet(latent_model_input, t, encoder_hidden_states=prompt_embeds, timestep_cond=timestep_cond,
                                               cross_attention_kwargs=self.cross_attention_kwargs, added_cond_kwargs=sdr_added,
                                               return_dict=False, **cn_kw)[0]
                    if do_cfg:
                        sdr_noise_pred_uncond, sdr_noise_pred_text = sdr_noise_pred.chunk(2)
                        sdr_noise_pred = sdr_noise_pred_uncond + self.guidance_scale * (sdr_noise_pred_text - sdr_noise_pred_uncond)
                    if do_cfg and self.guidance_rescale > 0.0:
                        sdr_noise_pred = rescale_noise_cfg(sdr_noise_pred, sdr_noise_pred_text, guidance_rescale=self.guidance_rescale)
                    # x0-prediction (dual.py:1071-1075), from the PRE-step latents
                    alphas_cumprod = self.scheduler.alphas_cumprod.to(sdr_noise_pred.device)[t].view(-1, 1, 1, 1)
                    sqrt_alpha_cumprod = alphas_cumprod.sqrt()
                    sqrt_one_minus_alpha_cumprod = (1 - alphas_cumprod).sqrt()
                    x0_latent = (latents - sqrt_one_minus_alpha_cumprod * sdr_noise_pred) / sqrt_alpha_cumprod
                    latents = self.scheduler.step(sdr_noise_pred, t, latents, **extra_step_kwargs, return_dict=False)[0]
                    if inpaint_mask is not None:
                        # diffusers' inpaint rule: the kept region returns to the picture at the next step's noise level (the picture
                        # itself at the last step); the GM UNet sees the clean picture where it is kept
                        kept = z0 if i == len(timesteps) - 1 else self.scheduler.add_noise(z0, noise, timesteps[i + 1:i + 2])
                        latents = (1 - inpaint_mask) * kept + inpaint_mask * latents
                        x0_latent = (1 - inpaint_mask) * z0 + inpaint_mask * x0_latent
                    gm_latent_input = torch.cat([x0_latent, gm_latents], dim=1)
                    gm_noise_pred = self.gm_unet(gm_latent_input, t, encoder_hidden_states=gm_prompt_embeds, timestep_cond=gm_timestep_cond,
                                                 cross_attention_kwargs=self.cross_attention_kwargs, added_cond_kwargs=gm_added,
                                                 return_dict=False)[0]
                    gm_latents = self.gm_scheduler.step(gm_noise_pred, t, gm_latents, **extra_step_kwargs, return_dict=False)[0]

                if self._step_probe is not None:
                    # test hook (tests/test_northstar_gpu.py): the reference's callback block is commented out
                    # (stable_diffusion_dual_unet.py:1095-1103) and its legacy callback sees the SDR latents only; the probe
                    # gets BOTH latents of iteration i after joining the two streams (this serialises them: not for timing)
                    if fused:
                        torch.cuda.synchronize(latents.device)
                    self._step_probe(i, latents, gm_latents)
                if i == len(timesteps) - 1 or ((i + 1) > num_warmup_steps and (i + 1) % self.scheduler.order == 0):
                    progress_bar.update()
                    if callback is not None and i % callback_steps == 0:
                        step_idx = i // getattr(self.scheduler, "order", 1)
                        callback(step_idx, t, latents)

        if fused:
            sdr_stream.wait_stream(gm_stream)  # join: the caller sees both results on its own stream
            gm_latents.record_stream(sdr_stream)
        self._check_f32_range("StableDiffusionDualUNetPipeline latents", self.unet, latents)
        self._check_f32_range("StableDiffusionDualUNetPipeline GM latents", self.gm_unet, gm_latents)
        if output_type == "latent":
            return (latents, gm_latents)
        sf = self.vae.config.scaling_factor
        sdr_image = self.vae.decode(latents / sf, return_dict=False, generator=generator)[0]
        gm_image = self.vae.decode(gm_latents / sf, return_dict=False, generator=generator)[0]
        self._check_f32_range("StableDiffusionDualUNetPipeline decoded images", self.vae, sdr_image, gm_image)
        do_denormalize = [True] * sdr_image.shape[0]
        sdr_out = self.image_processor.postprocess(sdr_image, output_type=output_type, do_denormalize=do_denormalize)
        gm_out = self.image_processor.postprocess(gm_image, output_type=output_type, do_denormalize=do_denormalize)
        self.maybe_free_model_hooks()
        return (sdr_out, gm_out)
