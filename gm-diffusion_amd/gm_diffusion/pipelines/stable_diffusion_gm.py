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
# Changes from that text: the LoRA / textual-inversion / IP-adapter branches are removed, the denoising loop, latent step,
# UNet / VAE calls and the decode tail are new (hand-written HIP kernels behind gm_diffusion.hip_ops).
"""
``StableDiffusionGMPipeline`` -- single 8-channel UNet that denoises the gain-map (GM) latent
conditioned on a given SDR latent.  Drop-in mirror of the reference class at
gm_diffusion/pipelines/stable_diffusion_gm.py:156 (constructor :202-213, ``__call__`` :780-1114):
same argument names, defaults, return types and errors.  The orchestration is host Python as in
the reference; what runs underneath is the MI355X path:

  * ``unet`` / ``vae`` are ``gm_diffusion.components`` models on hand-written HIP kernels;
  * with a ``PNDMScheduler`` and device tensors the per-step glue -- CFG combine, guidance
    rescale, PLMS update (:1062-1071) -- is ONE fused HIP kernel (``gmd_latent_step``) and the
    8-channel concat + CFG duplicate (:1045-1047) is folded into the UNet input pack kernel;
  * a guidance-embedded (LCM) UNet (config ``time_cond_proj_dim``) gets the guidance-scale embedding of :1028-1034 as
    ``timestep_cond`` and runs without the CFG duplicate; with ``LCMScheduler`` a step is ONE fused HIP kernel (``gmd_lcm_step``);
  * any other scheduler, or host tensors with a duck-typed UNet, takes the generic protocol path
    that executes the reference's torch expressions verbatim.

Behaviour notes kept from the reference: the latent channel count is forced to 4 and the latent
size is taken from ``sdr_latent`` (:1003-1015, ``height``/``width`` are ignored); unknown
``**kwargs`` are ignored (callers pass ``noise_level=``); per-call state lives on ``self``
(not re-entrant).  The textual-inversion / IP-adapter mixins of the diffusers base are not part
of this path (``ip_adapter_*`` raise ``NotImplementedError``).  LoRA: ``load_lora_weights`` loads named
adapters from local files, kept in factors and applied at run time (hip_ops.lora_update; several on one
projection: hip_ops.lora_update_stacked), ``set_adapters`` weighs them;
``cross_attention_kwargs['scale']`` is the scale of the call on top (nothing without an adapter).
"""
from __future__ import annotations

import functools
import inspect
import logging
import warnings
from typing import Any, Callable, Dict, List, Optional, Union

import torch

from ..components.configuration import FrozenDict
from ..components.image_processor import StableDiffusionPipelineOutput, VaeImageProcessor, randn_tensor
from .pipeline_utils import DiffusionPipeline

logger = logging.getLogger(__name__)


def rescale_noise_cfg(noise_cfg, noise_pred_text, guidance_rescale=0.0):
    """Reference: stable_diffusion_gm.py:71-94 (Section 3.4 of arXiv:2305.08891)."""
    std_text = noise_pred_text.std(dim=list(range(1, noise_pred_text.ndim)), keepdim=True)
    std_cfg = noise_cfg.std(dim=list(range(1, noise_cfg.ndim)), keepdim=True)
    noise_pred_rescaled = noise_cfg * (std_text / std_cfg)
    noise_cfg = guidance_rescale * noise_pred_rescaled + (1 - guidance_rescale) * noise_cfg
    return noise_cfg


def _per_call_lora_scale(call):
    """A pipeline ``__call__`` whose ``cross_attention_kwargs["scale"]`` holds for that call only (also when it raises)."""
    @functools.wraps(call)
    def wrapped(self, *args, **kwargs):
        try:
            return call(self, *args, **kwargs)
        finally:
            self._restore_lora_scale()

    return wrapped


def retrieve_timesteps(scheduler, num_inference_steps: Optional[int] = None, device=None,
                       timesteps: Optional[List[int]] = None, sigmas: Optional[List[float]] = None, **kwargs):
    """Reference: stable_diffusion_gm.py:97-153."""
    if timesteps is not None and sigmas is not None:
        raise ValueError("Only one of `timesteps` or `sigmas` can be passed. Please choose one to set custom values")
    if timesteps is not None:
        if "timesteps" not in set(inspect.signature(scheduler.set_timesteps).parameters.keys()):
            raise ValueError(
                f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                f" timestep schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(timesteps=timesteps, device=device, **kwargs)
        timesteps = scheduler.timesteps
        num_inference_steps = len(timesteps)
    elif sigmas is not None:
        if "sigmas" not in set(inspect.signature(scheduler.set_timesteps).parameters.keys()):
            raise ValueError(
                f"The current scheduler class {scheduler.__class__}'s `set_timesteps` does not support custom"
                f" sigmas schedules. Please check whether you are using the correct scheduler.")
        scheduler.set_timesteps(sigmas=sigmas, device=device, **kwargs)
        timesteps = scheduler.timesteps
        num_inference_steps = len(timesteps)
    else:
        scheduler.set_timesteps(num_inference_steps, device=device, **kwargs)
        timesteps = scheduler.timesteps
    return timesteps, num_inference_steps


class _GMPipelineBase(DiffusionPipeline):
    """Everything the GM and dual-UNet pipelines share (the reference duplicates it in three files)."""

    model_cpu_offload_seq = "text_encoder->image_encoder->unet->vae"
    _optional_components = ["safety_checker", "feature_extractor", "image_encoder"]
    _exclude_from_cpu_offload = ["safety_checker"]
    _callback_tensor_inputs = ["latents", "prompt_embeds", "negative_prompt_embeds"]
    _ip_adapter_supported = False  # image prompts (ip_adapter_image / ip_adapter_image_embeds): the dual-UNet pipeline only

    # ---- FreeU (diffusers' StableDiffusionMixin.enable_freeu / disable_freeu) -------------------------------------------------------
    def enable_freeu(self, s1, s2, b1, b2):
        """diffusers' ``enable_freeu``: FreeU on ``self.unet`` only, as the mixin does (the dual pipeline: the SDR UNet;
        ``pipe.gm_unet.enable_freeu(...)`` adapts the GM UNet).  See ``UNet2DConditionModel.enable_freeu``: all four values finite and
        > 0; a filter threshold other than 1, the "v2" variant, per-block settings and FreeU on the VAE or a ControlNet are not built."""
        if not hasattr(self, "unet"):
            raise ValueError("The pipeline must have `unet` for using FreeU.")
        self.unet.enable_freeu(s1=s1, s2=s2, b1=b1, b2=b2)

    def disable_freeu(self):
        """diffusers' ``disable_freeu``: ``self.unet`` back to the launches of a model that never had FreeU."""
        self.unet.disable_freeu()

    # ---- LoRA (diffusers' StableDiffusionLoraLoaderMixin, for LOCAL files; named adapters, kept in factors) -------------------------
    def load_lora_weights(self, path_or_state_dict, weight_name=None, subfolder=None, ignore_unsupported=False, adapter_name=None,
                          targets="attention", **kwargs):
        """diffusers' ``load_lora_weights`` for LOCAL files: a ``.safetensors`` file, a ``.bin`` / ``.pt`` torch pickle (read with
        ``weights_only=True``), a directory joined with ``subfolder`` and ``weight_name``, or the already-loaded state dict, in the
        PEFT, older diffusers or kohya key convention (components/lora.py).  Nothing is ever downloaded.  The adapter goes into
        ``self.unet`` (the dual pipeline: the SDR UNet; ``pipe.gm_unet.load_lora(...)`` adapts the GM UNet) and is applied at run
        time by one fused launch per targeted projection; targets that are not built raise unless ``ignore_unsupported``.
        ``targets``: "attention" (default: the eight attention projections of each transformer block) or "transformer" (also
        ff.net.0.proj, ff.net.2, proj_in and proj_out: kohya's default target set).  May be called repeatedly: each call adds one
        adapter under ``adapter_name`` (default ``default_0``, ``default_1``, ...); ``set_adapters`` weighs them."""
        from ..components import lora as _lora

        if kwargs:
            raise NotImplementedError(f"load_lora_weights: unsupported arguments {sorted(kwargs)} (local files only)")
        self.unet.load_lora(_lora.load_lora_file(path_or_state_dict, weight_name=weight_name, subfolder=subfolder),
                            ignore_unsupported=ignore_unsupported, targets=targets, adapter_name=adapter_name)

    def unload_lora_weights(self):
        """Drops ALL adapters of ``self.unet``."""
        self.unet.unload_lora()

    def fuse_lora(self, *args, **kwargs):
        raise NotImplementedError("fuse_lora: the adapter is kept in factors and applied at run time on purpose -- the device weights are "
                                  "derived layouts (stacked, interleaved, pre-split), a 16-bit merge loses the adapter's low bits, and the "
                                  "scale changes per call.  There is nothing to fuse or unfuse")

    unfuse_lora = fuse_lora

    def _lora_unets(self):
        """(component name, UNet) of every UNet that carries an adapter: ``unet``, and ``gm_unet`` where the pipeline has one."""
        out = []
        for name in ("unet", "gm_unet"):
            u = getattr(self, name, None)
            if u is not None and getattr(u, "has_lora", False):
                out.append((name, u))
        return out

    def set_adapters(self, adapter_names, adapter_weights=None):
        """diffusers' ``set_adapters``: the named adapters become active with ``adapter_weights`` (one float per name, default 1.0),
        every other loaded adapter gets weight 0.  Each UNet is addressed only for the names IT has loaded (the dual pipeline: an
        adapter loaded through ``pipe.gm_unet.load_lora`` is weighed by the same call); a name no UNet has loaded is a ``ValueError``
        (``components.lora.LoraAdapterError``: also the ``NotImplementedError`` this method raised while one adapter was all there was).
        Device tables only: no graph is captured anew.  ``cross_attention_kwargs={"scale": s}`` keeps its per-call meaning on top."""
        from ..components import lora as _lora

        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        if isinstance(adapter_weights, dict) or (isinstance(adapter_weights, (list, tuple)) and any(isinstance(w, dict) for w in adapter_weights)):
            raise NotImplementedError("set_adapters: per-block adapter weights (a dict per adapter) are not implemented: one float per adapter")
        if adapter_weights is None or not isinstance(adapter_weights, (list, tuple)):
            adapter_weights = [adapter_weights] * len(names)
        if len(adapter_weights) != len(names):
            raise ValueError(f"set_adapters: {len(adapter_weights)} weights for {len(names)} adapters")
        unets = self._lora_unets()
        loaded = {n for _, u in unets for n in u.list_adapters()}
        unknown = [n for n in names if n not in loaded]
        if unknown:
            raise _lora.LoraAdapterError(f"set_adapters: no adapter named {unknown} is loaded (loaded: {self.get_list_adapters()})")
        for _, u in unets:
            mine = [(n, w) for n, w in zip(names, adapter_weights) if n in u.list_adapters()]
            u.set_adapters([n for n, _ in mine], [w for _, w in mine])

    def delete_adapters(self, adapter_names):
        """diffusers' ``delete_adapters``: drops the named adapters from every UNet that has loaded them (unknown: ``ValueError``)."""
        from ..components import lora as _lora

        names = [adapter_names] if isinstance(adapter_names, str) else list(adapter_names)
        unets = self._lora_unets()
        loaded = {n for _, u in unets for n in u.list_adapters()}
        unknown = [n for n in names if n not in loaded]
        if unknown:
            raise _lora.LoraAdapterError(f"delete_adapters: no adapter named {unknown} is loaded (loaded: {self.get_list_adapters()})")
        for _, u in unets:
            mine = [n for n in names if n in u.list_adapters()]
            if mine:
                u.delete_adapters(mine)

    def get_active_adapters(self):
        """diffusers' ``get_active_adapters``: the adapters with a weight other than 0, in load order."""
        out = []
        for _, u in self._lora_unets():
            out.extend(n for n in u.active_adapters() if n not in out)
        return out

    def get_list_adapters(self):
        """diffusers' ``get_list_adapters``: ``{"unet": [...]}``, plus ``"gm_unet"`` when that UNet has any adapter."""
        unet = getattr(self, "unet", None)
        out = {"unet": unet.list_adapters() if unet is not None else []}
        gm = getattr(self, "gm_unet", None)
        if gm is not None and getattr(gm, "has_lora", False):
            out["gm_unet"] = gm.list_adapters()
        return out

    def disable_lora(self):
        """diffusers' ``disable_lora``: every adapter weight to 0, remembered; the launches stay (``UNet2DConditionModel.disable_lora``)."""
        for _, u in self._lora_unets():
            u.disable_lora()

    def enable_lora(self):
        """diffusers' ``enable_lora``: the weights ``disable_lora()`` remembered."""
        for _, u in self._lora_unets():
            u.enable_lora()

    def _apply_lora_scale(self, lora_scale):
        """``cross_attention_kwargs["scale"]`` of THIS call into the scale table of every UNet that carries an adapter, before the
        loop and outside any captured graph; ``_restore_lora_scale`` puts the models' own scale back when the call ends, so the key
        holds for one call, as in diffusers.  Without the key a call runs at the model's own scale: 1.0, unless the user changed it
        with ``unet.set_lora_scale``."""
        self._lora_scale_restore = []
        if lora_scale is None:
            return
        for name in ("unet", "gm_unet"):
            u = getattr(self, name, None)
            if u is not None and getattr(u, "has_lora", False):
                self._lora_scale_restore.append((u, u._lora_scale))
                u.set_lora_scale(float(lora_scale))

    def _restore_lora_scale(self):
        for u, s in getattr(self, "_lora_scale_restore", ()):
            if u.has_lora:
                u.set_lora_scale(s)
        self._lora_scale_restore = []

    def _init_common(self, vae, text_encoder, tokenizer, unet, scheduler, safety_checker, feature_extractor,
                     image_encoder, requires_safety_checker, **extra_modules):
        DiffusionPipeline.__init__(self)
        # stable_diffusion_gm.py:216-241: patch outdated scheduler configs
        if scheduler is not None and getattr(scheduler.config, "steps_offset", 1) != 1:
            warnings.warn(f"The configuration file of this scheduler: {scheduler} is outdated. `steps_offset` should be set to 1 "
                          f"instead of {scheduler.config.steps_offset}.", FutureWarning)
            new_config = dict(scheduler.config)
            new_config["steps_offset"] = 1
            scheduler._internal_dict = FrozenDict(new_config)
        if scheduler is not None and getattr(scheduler.config, "clip_sample", False) is True:
            warnings.warn(f"The configuration file of this scheduler: {scheduler} has not set the configuration `clip_sample`. "
                          "`clip_sample` should be set to False.", FutureWarning)
            new_config = dict(scheduler.config)
            new_config["clip_sample"] = False
            scheduler._internal_dict = FrozenDict(new_config)
        if safety_checker is None and requires_safety_checker:
            logger.warning(f"You have disabled the safety checker for {self.__class__} by passing `safety_checker=None`.")
        if safety_checker is not None and feature_extractor is None:
            raise ValueError("Make sure to define a feature extractor when loading {self.__class__} if you want to use the safety"
                             " checker. If you do not want to use the safety checker, you can pass `'safety_checker=None'` instead.")
        self._is_unet_config_sample_size_int = unet is not None and isinstance(unet.config.sample_size, int)
        modules = dict(vae=vae, text_encoder=text_encoder, tokenizer=tokenizer, unet=unet)
        modules.update(extra_modules)
        modules.update(scheduler=scheduler, safety_checker=safety_checker, feature_extractor=feature_extractor,
                       image_encoder=image_encoder)
        self.register_modules(**modules)
        self.vae_scale_factor = 2 ** (len(self.vae.config.block_out_channels) - 1) if getattr(self, "vae", None) else 8
        self.image_processor = VaeImageProcessor(vae_scale_factor=self.vae_scale_factor)
        self.register_to_config(requires_safety_checker=requires_safety_checker)

    # ---- prompt encoding (stable_diffusion_gm.py:334-514) ---------------------------------------
    def encode_prompt(self, prompt, device, num_images_per_prompt, do_classifier_free_guidance, negative_prompt=None,
                      prompt_embeds: Optional[torch.Tensor] = None, negative_prompt_embeds: Optional[torch.Tensor] = None,
                      lora_scale: Optional[float] = None, clip_skip: Optional[int] = None):
        if prompt is not None and isinstance(prompt, str):
            batch_size = 1
        elif prompt is not None and isinstance(prompt, list):
            batch_size = len(prompt)
        else:
            batch_size = prompt_embeds.shape[0]

        if prompt_embeds is None:
            text_inputs = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length,
                                         truncation=True, return_tensors="pt")
            text_input_ids = text_inputs.input_ids
            untruncated_ids = self.tokenizer(prompt, padding="longest", return_tensors="pt").input_ids
            if untruncated_ids.shape[-1] >= text_input_ids.shape[-1] and not torch.equal(text_input_ids, untruncated_ids):
                removed_text = self.tokenizer.batch_decode(untruncated_ids[:, self.tokenizer.model_max_length - 1: -1])
                logger.warning("The following part of your input was truncated because CLIP can only handle sequences up to"
                               f" {self.tokenizer.model_max_length} tokens: {removed_text}")
            if hasattr(self.text_encoder.config, "use_attention_mask") and self.text_encoder.config.use_attention_mask:
                attention_mask = text_inputs.attention_mask.to(device)
            else:
                attention_mask = None
            if clip_skip is None:
                prompt_embeds = self.text_encoder(text_input_ids.to(device), attention_mask=attention_mask)
                prompt_embeds = prompt_embeds[0]
            else:
                prompt_embeds = self.text_encoder(text_input_ids.to(device), attention_mask=attention_mask, output_hidden_states=True)
                prompt_embeds = prompt_embeds[-1][-(clip_skip + 1)]
                prompt_embeds = self.text_encoder.text_model.final_layer_norm(prompt_embeds)

        if self.text_encoder is not None:
            prompt_embeds_dtype = self.text_encoder.dtype
        elif self.unet is not None:
            prompt_embeds_dtype = self.unet.dtype
        else:
            prompt_embeds_dtype = prompt_embeds.dtype
        prompt_embeds = prompt_embeds.to(dtype=prompt_embeds_dtype, device=device)

        bs_embed, seq_len, _ = prompt_embeds.shape
        prompt_embeds = prompt_embeds.repeat(1, num_images_per_prompt, 1)
        prompt_embeds = prompt_embeds.view(bs_embed * num_images_per_prompt, seq_len, -1)

        if do_classifier_free_guidance and negative_prompt_embeds is None:
            uncond_tokens: List[str]
            if negative_prompt is None:
                uncond_tokens = [""] * batch_size
            elif prompt is not None and type(prompt) is not type(negative_prompt):
                raise TypeError(f"`negative_prompt` should be the same type to `prompt`, but got {type(negative_prompt)} !="
                                f" {type(prompt)}.")
            elif isinstance(negative_prompt, str):
                uncond_tokens = [negative_prompt]
            elif batch_size != len(negative_prompt):
                raise ValueError(f"`negative_prompt`: {negative_prompt} has batch size {len(negative_prompt)}, but `prompt`:"
                                 f" {prompt} has batch size {batch_size}. Please make sure that passed `negative_prompt` matches"
                                 " the batch size of `prompt`.")
            else:
                uncond_tokens = negative_prompt
            max_length = prompt_embeds.shape[1]
            uncond_input = self.tokenizer(uncond_tokens, padding="max_length", max_length=max_length, truncation=True,
                                          return_tensors="pt")
            if hasattr(self.text_encoder.config, "use_attention_mask") and self.text_encoder.config.use_attention_mask:
                attention_mask = uncond_input.attention_mask.to(device)
            else:
                attention_mask = None
            negative_prompt_embeds = self.text_encoder(uncond_input.input_ids.to(device), attention_mask=attention_mask)
            negative_prompt_embeds = negative_prompt_embeds[0]

        if do_classifier_free_guidance:
            seq_len = negative_prompt_embeds.shape[1]
            negative_prompt_embeds = negative_prompt_embeds.to(dtype=prompt_embeds_dtype, device=device)
            negative_prompt_embeds = negative_prompt_embeds.repeat(1, num_images_per_prompt, 1)
            negative_prompt_embeds = negative_prompt_embeds.view(batch_size * num_images_per_prompt, seq_len, -1)
        return prompt_embeds, negative_prompt_embeds

    def _encode_prompt(self, prompt, device, num_images_per_prompt, do_classifier_free_guidance, negative_prompt=None,
                       prompt_embeds=None, negative_prompt_embeds=None, lora_scale=None, **kwargs):
        """Deprecated concatenated form (stable_diffusion_gm.py:302-332)."""
        t = self.encode_prompt(prompt, device, num_images_per_prompt, do_classifier_free_guidance, negative_prompt,
                               prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, lora_scale=lora_scale, **kwargs)
        return torch.cat([t[1], t[0]])

    def run_safety_checker(self, image, device, dtype):
        if self.safety_checker is None:
            return image, None
        raise NotImplementedError("the safety checker is outside the GM-Diffusion hot path; pass safety_checker=None")

    def decode_latents(self, latents):
        """Deprecated helper (stable_diffusion_gm.py:599-608)."""
        latents = 1 / self.vae.config.scaling_factor * latents
        image = self.vae.decode(latents, return_dict=False)[0]
        image = self.image_processor.denormalize(image)
        return image.cpu().permute(0, 2, 3, 1).float().numpy()

    def prepare_extra_step_kwargs(self, generator, eta):
        """stable_diffusion_gm.py:610-625"""
        params = set(inspect.signature(self.scheduler.step).parameters.keys())
        extra = {}
        if "eta" in params:
            extra["eta"] = eta
        if "generator" in params:
            extra["generator"] = generator
        return extra

    def check_inputs(self, prompt, height, width, callback_steps, negative_prompt=None, prompt_embeds=None,
                     negative_prompt_embeds=None, ip_adapter_image=None, ip_adapter_image_embeds=None,
                     callback_on_step_end_tensor_inputs=None):
        """stable_diffusion_gm.py:627-694"""
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if callback_steps is not None and (not isinstance(callback_steps, int) or callback_steps <= 0):
            raise ValueError(f"`callback_steps` has to be a positive integer but is {callback_steps} of type"
                             f" {type(callback_steps)}.")
        if callback_on_step_end_tensor_inputs is not None and not all(
                k in self._callback_tensor_inputs for k in callback_on_step_end_tensor_inputs):
            raise ValueError(f"`callback_on_step_end_tensor_inputs` has to be in {self._callback_tensor_inputs}, but found "
                             f"{[k for k in callback_on_step_end_tensor_inputs if k not in self._callback_tensor_inputs]}")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                             " only forward one of the two.")
        elif prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        elif prompt is not None and (not isinstance(prompt, str) and not isinstance(prompt, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`:"
                             f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        if prompt_embeds is not None and negative_prompt_embeds is not None:
            if prompt_embeds.shape != negative_prompt_embeds.shape:
                raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                                 f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds`"
                                 f" {negative_prompt_embeds.shape}.")
        if ip_adapter_image is not None and ip_adapter_image_embeds is not None:
            raise ValueError("Provide either `ip_adapter_image` or `ip_adapter_image_embeds`. Cannot leave both `ip_adapter_image`"
                             " and `ip_adapter_image_embeds` defined.")
        if ip_adapter_image is not None or ip_adapter_image_embeds is not None:
            if not self._ip_adapter_supported:
                raise NotImplementedError(f"IP-Adapter conditioning is not implemented for {type(self).__name__}: image prompts run in "
                                          "StableDiffusionDualUNetPipeline (load_ip_adapter, ip_adapter_image / ip_adapter_image_embeds)")
            if ip_adapter_image_embeds is not None:  # stable_diffusion_dual_unet.py:688-696
                if not isinstance(ip_adapter_image_embeds, list):
                    raise ValueError(f"`ip_adapter_image_embeds` has to be of type `list` but is {type(ip_adapter_image_embeds)}")
                elif ip_adapter_image_embeds[0].ndim not in [3, 4]:
                    raise ValueError("`ip_adapter_image_embeds` has to be a list of 3D or 4D tensors but is"
                                     f" {ip_adapter_image_embeds[0].ndim}D")

    def prepare_latents(self, batch_size, num_channels_latents, height, width, dtype, device, generator, latents=None):
        """stable_diffusion_gm.py:696-716"""
        shape = (batch_size, num_channels_latents, int(height) // self.vae_scale_factor, int(width) // self.vae_scale_factor)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError(f"You have passed a list of generators of length {len(generator)}, but requested an effective batch"
                             f" size of {batch_size}. Make sure the batch size matches the length of the generators.")
        if latents is None:
            latents = randn_tensor(shape, generator=generator, device=device, dtype=dtype)
        else:
            latents = latents.to(device)
        latents = latents * self.scheduler.init_noise_sigma
        return latents

    def get_guidance_scale_embedding(self, w: torch.Tensor, embedding_dim: int = 512, dtype: torch.dtype = torch.float32) -> torch.Tensor:
        """stable_diffusion_gm.py:719-747: the sinusoidal embedding of the guidance scale that a guidance-embedded (LCM) UNet takes
        as ``timestep_cond``.  ``w``: 1-D tensor of ``guidance_scale - 1`` values.  Returns [len(w), embedding_dim] of ``dtype``:
        ``[sin | cos]`` of ``1000 * w * exp(-ln(10000) * i / (half - 1))``, i < half = embedding_dim // 2, with one zero column
        behind them when ``embedding_dim`` is odd."""
        if w.dim() != 1:
            raise ValueError(f"get_guidance_scale_embedding: `w` must be 1-D (got shape {tuple(w.shape)})")
        half = embedding_dim // 2
        scaled = w * 1000.0
        decay = torch.log(torch.tensor(10000.0)) / (half - 1)
        freqs = torch.exp(torch.arange(half, dtype=dtype) * -decay)
        angles = scaled.to(dtype)[:, None] * freqs[None, :]
        emb = torch.cat([angles.sin(), angles.cos()], dim=1)
        if embedding_dim % 2 == 1:
            emb = torch.nn.functional.pad(emb, (0, 1))
        return emb

    def _timestep_cond_for(self, unet, rows, device, dtype):
        """stable_diffusion_gm.py:1028-1034: the ``timestep_cond`` of ``unet`` -- the embedding of ``guidance_scale - 1``, one row
        per sample, at the UNet's own ``time_cond_proj_dim`` -- or None for a UNet without that projection."""
        dim = getattr(unet.config, "time_cond_proj_dim", None)
        if dim is None:
            return None
        w = torch.tensor(self.guidance_scale - 1).repeat(rows)
        return self.get_guidance_scale_embedding(w, embedding_dim=dim).to(device=device, dtype=dtype)

    # ---- properties (stable_diffusion_gm.py:749-778) ---------------------------------------------
    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def guidance_rescale(self):
        return self._guidance_rescale

    @property
    def clip_skip(self):
        return self._clip_skip

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1 and self.unet.config.time_cond_proj_dim is None

    @property
    def cross_attention_kwargs(self):
        return self._cross_attention_kwargs

    @property
    def num_timesteps(self):
        return self._num_timesteps

    @property
    def interrupt(self):
        return self._interrupt

    # ---- shared pieces of __call__ -------------------------------------------------------------
    @staticmethod
    def _check_f32_range(what, module, *tensors):
        """Range guard of the float32 matrix-core path (hip_ops.check_split_range): HIP float32 modules only."""
        if getattr(module, "dtype", None) == torch.float32 and hasattr(module, "_f32_mode"):
            from .. import hip_ops as ops

            ops.check_split_range(what, *tensors, module=module)

    def _latent_dtype(self, prompt_embeds, device):
        """Latents, scheduler state, CFG and x0 stay float32 on the HIP path (the documented cast point of the
        bf16 configuration: the UNet casts while packing its input); host tensors keep the reference's choice."""
        return torch.float32 if torch.device(device).type == "cuda" else prompt_embeds.dtype

    use_hip_graphs = True  # capture each UNet forward once per shape and replay it (device path only)
    # classifier-free guidance feeds the UNet the same latents twice (stable_diffusion_gm.py:1047): the layers in front of the
    # first cross-attention are evaluated once and duplicated (UNet2DConditionModel.forward_packed, ``cfg_shared``)
    share_cfg_prefix = True

    def _cfg_shared(self, unet, do_cfg):
        return bool(do_cfg and self.share_cfg_prefix and unet.supports_cfg_shared())

    def _graphs_ok(self):
        from .. import profiling

        return self.use_hip_graphs and profiling.active() is None

    def _use_fused(self, latents, unet, scheduler):
        from ..components.unet_2d_condition import UNet2DConditionModel

        # the scheduler says itself whether it has a fused device step (components.schedulers: every class there does)
        return latents.is_cuda and getattr(scheduler, "has_fused_step", False) and isinstance(unet, UNet2DConditionModel)

    @staticmethod
    def _pack_div(scheduler, timestep):
        """What the fused loops pass as ``div`` to ``pack_input``: None for the variance-preserving schedulers (their
        ``scale_model_input`` is the identity: the plain pack, unchanged), the current step's ``(sigma**2 + 1) ** 0.5`` for a
        sigma-space scheduler (Euler, Euler ancestral, LMS), whose ``scale_model_input`` (stable_diffusion_gm.py:1048) is folded into the
        pack kernel."""
        return scheduler.input_divisor(timestep) if getattr(scheduler, "sigma_space", False) else None

    PREDRAW_NOISE_BYTES = 512 << 20  # ceiling of the pre-drawn scheduler noise (host pinned copy + device copy)

    @staticmethod
    def _predraw_step_noise(schedulers, ts_host, shape, generator, device, eta=0.0, first=None):
        """Stochastic schedulers on the fused path with a CPU generator: draw the variance noise of EVERY step now, in exactly
        the order the loop would consume the generator (per iteration: the schedulers in the order given -- SDR before GM,
        stable_diffusion_dual_unet.py:1077, 1093), and move it to the device in one asynchronous copy.  A draw inside the
        loop is a host-side randn + synchronous copy per step, which stops the host from running ahead of the GPU
        (bench.py --scheduler ddpm: 3.67 -> 4.59 images/s).  Returns one list of per-step tensors (or None) per scheduler,
        or None when there is nothing to pre-draw (deterministic scheduler, device generator, global RNG) or when the noise
        of all steps would exceed PREDRAW_NOISE_BYTES (DDPM's default 1000 steps at 1024x1024, batch 8, two schedulers is
        ~4 GB on the host AND on the device): the loop then draws per step, as the reference does.
        DDIM draws iff ``eta`` > 0, then at every step (the last included): every (step, scheduler) is a slot.  So does a
        ``DPMSolverMultistepScheduler`` with the SDE algorithm, and ``EulerAncestralDiscreteScheduler`` always; a deterministic
        scheduler (``EulerDiscreteScheduler``, ``LMSDiscreteScheduler`` and ``UniPCMultistepScheduler`` among them) has nothing to pre-draw.  ``LCMScheduler`` draws
        at every step but the last, as DDPM does.
        ``first``: per scheduler, the iteration it takes its first step at (None: every scheduler steps from iteration 0).  The dual
        pipeline's img2img loop steps the GM scheduler alone for the first iterations: per iteration the order is still the
        schedulers' order, over those that step.
        Difference from the reference under ``interrupt``: the pre-draw has already advanced the caller's generator for the
        steps an interrupt later skips; the reference would not have consumed those draws."""
        if generator is None or not all(getattr(s_, "predraws_noise", False) for s_ in schedulers):
            return None
        gens = generator if isinstance(generator, list) else [generator]
        if any(g_.device.type != "cpu" for g_ in gens):
            return None
        slots = [(i, k) for i, t in enumerate(ts_host) for k, s_ in enumerate(schedulers)
                 if (first is None or i >= first[k]) and s_.draws_noise(t, eta)]
        if not slots:
            return None
        nbytes = 4 * len(slots)
        for d in shape:
            nbytes *= int(d)
        if nbytes > StableDiffusionGMPipeline.PREDRAW_NOISE_BYTES:
            return None
        host = torch.stack([randn_tensor(shape, generator=generator, device="cpu", dtype=torch.float32) for _ in slots])
        on_gpu = torch.device(device).type == "cuda"
        dev = host.pin_memory().to(device, non_blocking=True) if (host.numel() and on_gpu) else host.to(device)
        out = [[None] * len(ts_host) for _ in schedulers]
        for n, (i, k) in enumerate(slots):
            out[k][i] = dev[n]
        return out

    @staticmethod
    def _fused_step_kwargs(extra_step_kwargs):
        """What ``scheduler.fused_step`` takes of the reference's ``extra_step_kwargs``: the generator (stochastic
        schedulers draw their noise from it in call order, stable_diffusion_dual_unet.py:1077, 1093) and ``eta``, which
        ``prepare_extra_step_kwargs`` includes only for a scheduler whose ``step`` takes it (DDIM)."""
        return {k: extra_step_kwargs[k] for k in ("generator", "eta") if k in extra_step_kwargs}

    def _default_hw(self, height, width):
        if not height or not width:
            height = self.unet.config.sample_size if self._is_unet_config_sample_size_int else self.unet.config.sample_size[0]
            width = self.unet.config.sample_size if self._is_unet_config_sample_size_int else self.unet.config.sample_size[1]
            height, width = height * self.vae_scale_factor, width * self.vae_scale_factor
        return height, width

    @staticmethod
    def _pop_legacy_callbacks(kwargs):
        callback = kwargs.pop("callback", None)
        callback_steps = kwargs.pop("callback_steps", None)
        if callback is not None:
            warnings.warn("Passing `callback` as an input argument to `__call__` is deprecated, consider using `callback_on_step_end`", FutureWarning)
        if callback_steps is not None:
            warnings.warn("Passing `callback_steps` as an input argument to `__call__` is deprecated, consider using `callback_on_step_end`", FutureWarning)
        return callback, callback_steps


class StableDiffusionGMPipeline(_GMPipelineBase):
    def __init__(self, vae, text_encoder, tokenizer, unet, scheduler, safety_checker, feature_extractor,
                 image_encoder=None, requires_safety_checker: bool = True):
        self._init_common(vae, text_encoder, tokenizer, unet, scheduler, safety_checker, feature_extractor, image_encoder,
                          requires_safety_checker)

    @_per_call_lora_scale
    @torch.no_grad()
    def __call__(
        self,
        sdr_latent: torch.Tensor,
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
        lora_scale = self.cross_attention_kwargs.get("scale", None) if self.cross_attention_kwargs is not None else None
        self._apply_lora_scale(lora_scale)
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, device, num_images_per_prompt, self.do_classifier_free_guidance, negative_prompt,
            prompt_embeds=prompt_embeds, negative_prompt_embeds=negative_prompt_embeds, lora_scale=lora_scale,
            clip_skip=self.clip_skip)
        if self.do_classifier_free_guidance:
            prompt_embeds = torch.cat([negative_prompt_embeds, prompt_embeds])

        timesteps, num_inference_steps = retrieve_timesteps(self.scheduler, num_inference_steps, device, timesteps, sigmas)

        # gm.py:1003-1015: latent channels forced to 4, latent size taken from sdr_latent
        num_channels_latents = 4
        latents = self.prepare_latents(batch_size * num_images_per_prompt, num_channels_latents, sdr_latent.shape[-2] * 8,
                                       sdr_latent.shape[-1] * 8, self._latent_dtype(prompt_embeds, device), device, generator, latents)
        extra_step_kwargs = self.prepare_extra_step_kwargs(generator, eta)
        # gm.py:1028-1034: the guidance scale goes INTO a guidance-embedded (LCM) UNet, which then runs without the CFG duplicate
        timestep_cond = self._timestep_cond_for(self.unet, batch_size * num_images_per_prompt, device, latents.dtype)

        num_warmup_steps = len(timesteps) - num_inference_steps * self.scheduler.order
        self._num_timesteps = len(timesteps)
        do_cfg = self.do_classifier_free_guidance
        fused = self._use_fused(latents, self.unet, self.scheduler)
        if fused:
            ctx = self.unet.prepare_context(prompt_embeds)
            # constant over the loop: written once into the persistent buffer the (captured) forward reads
            self.unet.set_timestep_cond(timestep_cond, (2 if do_cfg else 1) * latents.shape[0])
            sdr_f32 = sdr_latent.to(device=latents.device, dtype=torch.float32).contiguous()
            # host copy: no device sync inside the loop; int64 timesteps stay ints, the float32 (possibly fractional) timesteps of
            # a sigma-space scheduler stay floats -- never truncated
            ts_host = timesteps.tolist()
            ts_dev = timesteps.to(device=latents.device, dtype=torch.float32)
            hw = latents.shape[-2:]
            shared = self._cfg_shared(self.unet, do_cfg)
            nb = (2 if do_cfg else 1) * latents.shape[0]
            pre = self._predraw_step_noise([self.scheduler], ts_host, latents.shape, generator, latents.device,
                                           eta=extra_step_kwargs.get("eta", 0.0))
            graph = self.unet.graphed_forward(nb, hw[0], hw[1], ctx, cfg_shared=shared) if self._graphs_ok() else None

        with self.progress_bar(total=num_inference_steps) as progress_bar:
            for i, t in enumerate(timesteps):
                if self.interrupt:
                    continue
                if fused:
                    # concat(sdr, gm) + CFG duplicate + cast fused into the input pack; CFG/rescale/PLMS in one kernel
                    div = self._pack_div(self.scheduler, ts_host[i])  # gm.py:1048 scales the concatenated tensor: both halves
                    x = self.unet.pack_input((sdr_f32, latents), dup=2 if (do_cfg and not shared) else 1, out=graph.x if graph else None,
                                             **({"div": (div, div)} if div is not None else {}))
                    self.unet.set_timestep_from(ts_dev, i)
                    noise_pred = graph.replay() if graph else self.unet.forward_packed(x, nb, hw[0], hw[1], ctx, cfg_shared=shared)
                    latents, _ = self.scheduler.fused_step(noise_pred, ts_host[i], latents, do_cfg, self.guidance_scale,
                                                           self.guidance_rescale if do_cfg else 0.0,
                                                           **self._fused_step_kwargs(extra_step_kwargs),
                                                           **({"noise": pre[0][i]} if pre else {}))
                else:
                    cat_latents = torch.cat([sdr_latent, latents], dim=1)
                    latent_model_input = torch.cat([cat_latents] * 2) if do_cfg else cat_latents
                    latent_model_input = self.scheduler.scale_model_input(latent_model_input, t)
                    noise_pred = self.unet(latent_model_input, t, encoder_hidden_states=prompt_embeds, timestep_cond=timestep_cond,
                                           cross_attention_kwargs=self.cross_attention_kwargs, added_cond_kwargs=None,
                                           return_dict=False)[0]
                    if do_cfg:
                        noise_pred_uncond, noise_pred_text = noise_pred.chunk(2)
                        noise_pred = noise_pred_uncond + self.guidance_scale * (noise_pred_text - noise_pred_uncond)
                    if do_cfg and self.guidance_rescale > 0.0:
                        noise_pred = rescale_noise_cfg(noise_pred, noise_pred_text, guidance_rescale=self.guidance_rescale)
                    latents = self.scheduler.step(noise_pred, t, latents, **extra_step_kwargs, return_dict=False)[0]

                if callback_on_step_end is not None:
                    callback_kwargs = {}
                    for k in callback_on_step_end_tensor_inputs:
                        callback_kwargs[k] = locals()[k]
                    callback_outputs = callback_on_step_end(self, i, t, callback_kwargs)
                    latents = callback_outputs.pop("latents", latents)
                    new_pe = callback_outputs.pop("prompt_embeds", prompt_embeds)
                    if new_pe is not prompt_embeds:
                        prompt_embeds = new_pe
                        if fused:
                            ctx = self.unet.prepare_context(prompt_embeds)
                            self.unet.update_context(ctx)
                    negative_prompt_embeds = callback_outputs.pop("negative_prompt_embeds", negative_prompt_embeds)

                if i == len(timesteps) - 1 or ((i + 1) > num_warmup_steps and (i + 1) % self.scheduler.order == 0):
                    progress_bar.update()
                    if callback is not None and i % callback_steps == 0:
                        step_idx = i // getattr(self.scheduler, "order", 1)
                        callback(step_idx, t, latents)

        self._check_f32_range("StableDiffusionGMPipeline latents", self.unet, latents)
        if not output_type == "latent":
            image = self.vae.decode(latents / self.vae.config.scaling_factor, return_dict=False, generator=generator)[0]
            self._check_f32_range("StableDiffusionGMPipeline decoded image", self.vae, image)
            image, has_nsfw_concept = self.run_safety_checker(image, device, prompt_embeds.dtype)
        else:
            image = latents
            has_nsfw_concept = None
        if has_nsfw_concept is None:
            do_denormalize = [True] * image.shape[0]
        else:
            do_denormalize = [not has_nsfw for has_nsfw in has_nsfw_concept]
        image = self.image_processor.postprocess(image, output_type=output_type, do_denormalize=do_denormalize)
        self.maybe_free_model_hooks()
        if not return_dict:
            return (image, has_nsfw_concept)
        return StableDiffusionPipelineOutput(images=image, nsfw_content_detected=has_nsfw_concept)
