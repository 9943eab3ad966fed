"""
Host-side helpers the reference pipelines take from diffusers: ``randn_tensor``
(stable_diffusion_gm.py:709-710), ``VaeImageProcessor.postprocess`` (:1106),
``StableDiffusionPipelineOutput`` (:1114).
"""
from __future__ import annotations

from dataclasses import dataclass, fields
from typing import Any, List, Optional, Union

import numpy as np
import torch

from .. import hip_ops as ops


def randn_tensor(shape, generator=None, device=None, dtype=None, layout=None):
    """diffusers.utils.torch_utils.randn_tensor: draw on the generator's device (CPU generators give
    device-independent, shard-independent noise), then move.  A list of generators draws one
    sample per generator."""
    device = torch.device(device) if device is not None else torch.device("cpu")
    batch = shape[0]
    layout = layout or torch.strided
    rand_device = device
    if generator is not None:
        gen_dev = generator.device.type if not isinstance(generator, list) else generator[0].device.type
        if gen_dev != device.type and gen_dev == "cpu":
            rand_device = torch.device("cpu")
        elif gen_dev != device.type and gen_dev == "cuda":
            raise ValueError(f"Cannot generate a {device} tensor from a generator of type {gen_dev}.")
    if isinstance(generator, list) and len(generator) == 1:
        generator = generator[0]
    if isinstance(generator, list):
        sub = (1,) + tuple(shape[1:])
        lat = [torch.randn(sub, generator=generator[i], device=rand_device, dtype=dtype, layout=layout) for i in range(batch)]
        return torch.cat(lat, dim=0).to(device)
    return torch.randn(tuple(shape), generator=generator, device=rand_device, dtype=dtype, layout=layout).to(device)


class _Output:
    """dataclass with tuple-style indexing (diffusers ``BaseOutput``)."""

    def __getitem__(self, k):
        if isinstance(k, str):
            return getattr(self, k)
        return tuple(getattr(self, f.name) for f in fields(self) if getattr(self, f.name) is not None)[k]

    def to_tuple(self):
        return tuple(getattr(self, f.name) for f in fields(self))


@dataclass
class StableDiffusionPipelineOutput(_Output):
    images: Any
    nsfw_content_detected: Optional[List[bool]]


@dataclass
class UNetOutput(_Output):
    sample: torch.Tensor


class VaeImageProcessor:
    def __init__(self, vae_scale_factor=8, do_normalize=True):
        self.vae_scale_factor = vae_scale_factor
        self.config = type("cfg", (), {"vae_scale_factor": vae_scale_factor, "do_normalize": do_normalize})()

    @staticmethod
    def denormalize(images):
        """``(images / 2 + 0.5).clamp(0, 1)`` -- HIP kernel for device tensors."""
        if torch.is_tensor(images) and images.is_cuda:
            x = images.contiguous()
            if x.dtype != torch.float32:
                x = ops.cast(x, torch.float32)
            return ops.tmo(x, 4)
        return (images / 2 + 0.5).clamp(0, 1)

    @staticmethod
    def pt_to_numpy(images):
        return images.cpu().permute(0, 2, 3, 1).float().numpy()

    @staticmethod
    def numpy_to_pil(images):
        from PIL import Image

        if images.ndim == 3:
            images = images[None, ...]
        images = (images * 255).round().astype("uint8")
        if images.shape[-1] == 1:
            return [Image.fromarray(im.squeeze(), mode="L") for im in images]
        return [Image.fromarray(im) for im in images]

    @staticmethod
    def normalize(images):
        """diffusers' ``2.0 * images - 1.0``: [0, 1] -> [-1, 1]."""
        return 2.0 * images - 1.0

    def preprocess(self, image, height=None, width=None):
        """The img2img input as the VAE takes it: float32 NCHW in [-1, 1].  Taken: a float tensor [3, H, W] / [B, 3, H, W] in
        [0, 1]; a uint8 tensor or numpy array [H, W, 3] / [B, H, W, 3]; a PIL image; a list of any of these (one image each).
        Unlike diffusers' ``preprocess`` this only normalises and lays out NCHW: nothing is resized, and an image that is not
        ``height`` x ``width`` is a ValueError (``hdr.prepare_sdr`` resizes and crops a picture on the device)."""
        if isinstance(image, (list, tuple)):
            if len(image) == 0:
                raise ValueError("`image` is an empty list")
            return torch.cat([self.preprocess(im, height, width) for im in image], 0)
        if not torch.is_tensor(image):
            arr = np.array(image)  # (a copy: a PIL image's buffer is read-only)
            if arr.dtype != np.uint8:
                raise ValueError(f"`image` as an array or PIL image must be uint8 RGB (got dtype {arr.dtype}); pass floats as a"
                                 " [B, 3, H, W] tensor in [0, 1]")
            image = torch.from_numpy(np.ascontiguousarray(arr))
        if image.dtype == torch.uint8:
            if image.dim() == 3:
                image = image[None]
            if image.dim() != 4 or image.shape[-1] != 3:
                raise ValueError(f"a uint8 `image` must be [H, W, 3] or [B, H, W, 3] (got {tuple(image.shape)})")
            image = image.permute(0, 3, 1, 2).to(torch.float32) / 255.0
        elif image.is_floating_point():
            if image.dim() == 3:
                image = image[None]
            if image.dim() != 4 or image.shape[1] != 3:
                raise ValueError(f"a float `image` must be [3, H, W] or [B, 3, H, W] in [0, 1] (got {tuple(image.shape)})")
            image = image.to(torch.float32)
        else:
            raise ValueError(f"`image` must be uint8 or floating point (got {image.dtype})")
        if height is not None and width is not None and tuple(image.shape[-2:]) != (int(height), int(width)):
            raise ValueError(f"`image` is {image.shape[-2]} x {image.shape[-1]} but this call is {height} x {width} (height x width);"
                             " nothing is resized here: resize and crop the picture with gm_diffusion.hdr.prepare_sdr first")
        image = self.normalize(image) if self.config.do_normalize else image
        return image.contiguous()

    def postprocess(self, image, output_type="pil", do_denormalize=None):
        if not torch.is_tensor(image):
            raise ValueError(f"Input for postprocessing is in incorrect format: {type(image)}. Only pytorch tensor is supported")
        if output_type not in ("latent", "pt", "np", "pil"):
            output_type = "np"
        if output_type == "latent":
            return image
        if do_denormalize is None:
            do_denormalize = [self.config.do_normalize] * image.shape[0]
        if all(do_denormalize):
            image = self.denormalize(image)
        elif any(do_denormalize):
            image = torch.stack([self.denormalize(image[i:i + 1])[0] if do_denormalize[i] else image[i] for i in range(image.shape[0])])
        if output_type == "pt":
            return image
        image = self.pt_to_numpy(image)
        if output_type == "np":
            return image
        return self.numpy_to_pil(image)
