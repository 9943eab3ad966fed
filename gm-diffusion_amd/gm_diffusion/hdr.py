"""
The Stage-3 tail as ONE device-side pass: decode both latents, post-process, quantise the PNG
bytes, recompose HDR with Eq. 1 and scale for the Radiance writer.  This is the composition the
reference's CLI performs on the host after the pipeline returns latents
(scripts/inference/generate_hdr.py:225-265, scripts/inference/experiments/formal_improved.py:272-303):

    sdr = vae.decode(1/sf * sdr_latent); sdr = (sdr/2+0.5).clamp(0,1)        gen.py:225-228
    gm  = vae.decode(1/sf * gm_latent);  gm  = (gm/2+0.5).clamp(0,1)         gen.py:230-233
    PNG bytes (x*255).astype(uint8)                                          gen.py:244-245
    hdr = apply_gm_to_sdr(sdr, gm, qmax=99)   [numpy variant: no clamp]      fi.py:34-45, gen.py:256-259
    file = hdr/(qmax+1)                                                      gen.py:27-29

Here the two decodes run on the HIP VAE (channels-last) and everything after them is the single
``gmd_hdr_tail`` kernel reading the decoder's float32 [B,H*W,4] image directly (no transpose, no
host round trip).  Outputs stay on the device as [B,H,W,3] tensors; ``to_host`` gives the numpy
arrays the reference scripts hold.
"""
from __future__ import annotations

import torch

from . import hip_ops as ops


_TAIL_WANT = ("sdr", "gm", "sdr_u8", "gm_u8", "hdr", "hdr_file", "hdr_u16")


def _decode_nhwc(vae, *latents):
    """The given latents through the (shared) decoder as ONE batch: half the launches, fuller grids.  Returns the float32
    [n*B, H*W, 4] image, H, W."""
    inv = 1.0 / vae.config.scaling_factor
    both = torch.cat([_f32(x) for x in latents], 0) if len(latents) > 1 else _f32(latents[0])
    dec, H, W = vae.decode_nhwc(ops.tmo(both, 5, mu=inv))
    if vae.dtype == torch.float32:
        ops.check_split_range("decode_to_hdr: decoded images", dec, module=vae)  # the VAE's activations are the widest of the path
    return dec, H, W


def decode_to_hdr(vae, sdr_latent, gm_latent, qmax=99.0, eps=1 / 64, clamp=False, want=_TAIL_WANT, out_size=None, source_u8=None):
    """Returns a dict of device tensors [B,H,W,3]: sdr/gm (float32 in [0,1]), sdr_u8/gm_u8 (truncated PNG bytes),
    hdr (Eq. 1), hdr_file (= hdr/(qmax+1)), hdr_u16 (round-half-even codes of clamp(hdr_file)).

    ``out_size`` = (H, W): the outputs are written at that size instead of the decoder's -- both decoded images are bilinearly
    resampled onto it inside the one tail kernel (``gmd_hdr_tail_resized``; what the reference's drivers do with two ``cv2.resize``
    calls before ``apply_gm_to_sdr``, demo_training_loop.py:291-304), and ``"hdr_rgbe"`` ([B,H,W,4] uint8 Radiance pixels of
    hdr_file, ready for ``save_hdr_image``) becomes an allowed key of ``want``.  ``source_u8``: a uint8 [B,H,W,3] picture that takes
    the place of the decoded SDR (generate_hdr.py:262-265, ``original_hdr_image``); its size is the output size and
    ``sdr_latent`` may be None (only the gain map is decoded then)."""
    if out_size is None and source_u8 is None:
        if "hdr_rgbe" in want:
            raise ValueError("decode_to_hdr: 'hdr_rgbe' is an output of the resized tail: pass out_size or source_u8")
        B = sdr_latent.shape[0]
        dec, H, W = _decode_nhwc(vae, sdr_latent, gm_latent)  # [2B, H*W, 4] float32
        return ops.hdr_tail(dec[:B], dec[B:], 2, B, H, W, qmax=qmax, eps=eps, clamp=clamp, want=want)
    B = gm_latent.shape[0]
    if source_u8 is not None:
        size = tuple(int(v) for v in source_u8.shape[1:3])
        if out_size is not None and tuple(int(v) for v in out_size) != size:
            raise ValueError(f"decode_to_hdr: out_size {tuple(out_size)} differs from the source picture's {size}")
        dec, H, W = _decode_nhwc(vae, gm_latent)
        return ops.hdr_tail_resized(source_u8.contiguous(), dec, 2, size, gm_hw=(H, W), qmax=qmax, eps=eps, clamp=clamp,
                                    source_u8=True, want=want)
    dec, H, W = _decode_nhwc(vae, sdr_latent, gm_latent)
    return ops.hdr_tail_resized(dec[:B], dec[B:], 2, out_size, sdr_hw=(H, W), gm_hw=(H, W), qmax=qmax, eps=eps, clamp=clamp, want=want)


def recompose(sdr_dec, gm_dec, qmax=99.0, eps=1 / 64, clamp=False, out_size=None, source_u8=None, **kw):
    """Same tail for already-decoded NCHW images in [-1,1] (e.g. ``vae.decode(...)[0]``).  ``out_size`` / ``source_u8`` as in
    ``decode_to_hdr``; the two images may then differ in size, and ``sdr_dec`` may be None with ``source_u8``."""
    if out_size is None and source_u8 is None:
        B, _, H, W = sdr_dec.shape
        return ops.hdr_tail(sdr_dec.contiguous(), gm_dec.contiguous(), 0, B, H, W, qmax=qmax, eps=eps, clamp=clamp, **kw)
    if source_u8 is not None:
        size = tuple(int(v) for v in source_u8.shape[1:3])
        if out_size is not None and tuple(int(v) for v in out_size) != size:
            raise ValueError(f"recompose: out_size {tuple(out_size)} differs from the source picture's {size}")
        return ops.hdr_tail_resized(source_u8.contiguous(), gm_dec.contiguous(), 0, size, qmax=qmax, eps=eps, clamp=clamp, source_u8=True, **kw)
    return ops.hdr_tail_resized(sdr_dec.contiguous(), gm_dec.contiguous(), 0, out_size, qmax=qmax, eps=eps, clamp=clamp, **kw)


def prepare_sdr(images_u8, size, dtype=torch.float32):
    """uint8 [B,h,w,3] device pictures -> the VAE encoder's input [B,3,H,W] at ``size`` = (H, W): Resize(BILINEAR, antialiased) +
    ToTensor + Normalize([0.5], [0.5]) of the reference's ``val_transforms`` (demo_training_loop.py:205-211) as one kernel."""
    return ops.prepare_sdr(images_u8.contiguous(), size, dtype)


def sdr_to_hdr(pipe, images_u8, size, prompt=None, num_inference_steps=50, generator=None, qmax=99, eps=1 / 64, clamp=False,
               original=False, want=("hdr", "hdr_file", "hdr_rgbe"), **pipe_kwargs):
    """The loop body of the reference's Stage-3 drivers (demo_training_loop.py:223-304) as one call.  ``images_u8``: uint8
    [B,h,w,3] source pictures on the device; ``size`` = (H, W): the model's working size (multiples of 8).
      1. prepare: resize + normalise straight into the encoder's channels-last input                       :205-211, 230
      2. ``vae.encode(...).latent_dist.sample(generator)`` times the scaling factor                         :237-238
      3. the GM pipeline with ``output_type="latent"`` (``pipe_kwargs``: prompt_embeds, guidance_scale, ...) :242-248
      4. both decodes, gain map and decoded SDR resampled to the source size, Eq. 1                          :255-263, 291-299
    Returns the ``want`` outputs at the source size (``hdr`` is the decoded SDR recomposed) and, with ``original=True``,
    ``original_hdr`` / ``original_hdr_file`` / ``original_hdr_rgbe``: the same gain map applied to the source pixels themselves
    (generate_hdr.py:262-265).  ``sdr_latent`` and ``gm_latent`` are returned too."""
    vae = pipe.vae
    B, h, w = (int(v) for v in images_u8.shape[:3])
    H, W = int(size[0]), int(size[1])
    cp, dt = vae.encoder_input_spec()
    x = ops.prepare_sdr(images_u8.contiguous(), (H, W), dt, layout="nhwc", cp=cp)
    sdr_latent = vae.encode_nhwc(x, H, W).latent_dist.sample(generator) * vae.config.scaling_factor
    gm_latent = pipe(sdr_latent, prompt=prompt, num_inference_steps=num_inference_steps, generator=generator, output_type="latent",
                     **pipe_kwargs).images
    dec, Hd, Wd = _decode_nhwc(vae, sdr_latent, gm_latent)
    out = ops.hdr_tail_resized(dec[:B], dec[B:], 2, (h, w), sdr_hw=(Hd, Wd), gm_hw=(Hd, Wd), qmax=qmax, eps=eps, clamp=clamp, want=want)
    if original:
        keys = tuple(k for k in want if k.startswith("hdr")) or ("hdr",)
        org = ops.hdr_tail_resized(images_u8.contiguous(), dec[B:], 2, (h, w), gm_hw=(Hd, Wd), qmax=qmax, eps=eps, clamp=clamp,
                                   source_u8=True, want=keys)
        out.update({"original_" + k: v for k, v in org.items()})
    out["sdr_latent"], out["gm_latent"] = sdr_latent, gm_latent
    return out


def to_host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def _f32(x):
    x = x.contiguous()
    return x if x.dtype == torch.float32 else ops.cast(x, torch.float32)


# ------------------------------------------------------------------------------------------------
# file writers: the reference uses cv2.imwrite("*.hdr") / PIL; cv2 is absent here
# ------------------------------------------------------------------------------------------------
def rgbe_scanlines(px, compression="rle"):
    """Bytes that follow the header of a Radiance picture for RGBE pixels ``px`` ([H, W, 4] uint8 host array): run-length
    framed scanlines ("rle": what OpenCV's encoder behind cv2.imwrite writes by default; host function gmd_rgbe_rle_encode of
    the C ABI) or flat pixels ("none": cv2's IMWRITE_HDR_COMPRESSION_NONE)."""
    import ctypes

    import numpy as np

    from ._native import check, lib
    px = np.ascontiguousarray(px, dtype=np.uint8)
    if px.ndim != 3 or px.shape[-1] != 4:
        raise ValueError("rgbe_scanlines expects [H, W, 4] bytes")
    if compression == "none":
        return px.tobytes()
    if compression != "rle":
        raise ValueError("compression must be 'rle' or 'none'")
    h, w = int(px.shape[0]), int(px.shape[1])
    cap = int(lib().gmd_rgbe_rle_bound(h, w))
    out = np.empty(max(cap, 1), np.uint8)
    n = ctypes.c_int64(0)
    check(lib().gmd_rgbe_rle_encode(px.ctypes.data, h, w, out.ctypes.data, cap, ctypes.addressof(n)), "gmd_rgbe_rle_encode")
    return out[: n.value].tobytes()


def save_hdr_image(hdr_file_rgb, path, compression="rle"):
    """Write one Radiance RGBE picture.  ``hdr_file_rgb``: [H,W,3] float32 device tensor, already divided by
    (qmax+1) and in RGB order (= ``out['hdr_file'][i]``); this is what the reference's ``save_hdr_image``
    (generate_hdr.py:27-30) hands to ``cv2.imwrite`` after its BGR swap.  Pixels are encoded on the device
    (gmd_rgbe_encode); scanlines are run-length framed on the host like OpenCV's writer does by default
    (``compression="none"`` writes them flat).  cv2 is absent in this image: header text and framing follow the published
    Radiance format, not a byte comparison with cv2's output.
    Negative values (possible with the unclamped Eq. 1) are stored as 0: RGBE has no sign.
    An already-encoded [H,W,4] uint8 tensor (= ``out['hdr_rgbe'][i]`` of the resized tail) is written as it is: only the bytes
    cross to the host, never a full-size float image."""
    x = hdr_file_rgb.contiguous()
    if x.dim() == 3 and x.shape[-1] == 4 and x.dtype == torch.uint8:
        px = x.cpu().numpy()
    elif x.dim() != 3 or x.shape[-1] != 3:
        raise ValueError("save_hdr_image expects [H, W, 3] float or [H, W, 4] uint8")
    else:
        px = ops.rgbe_encode(_f32(x)).cpu().numpy()
    h, w = x.shape[0], x.shape[1]
    with open(path, "wb") as f:
        f.write(b"#?RADIANCE\nFORMAT=32-bit_rle_rgbe\n\n")
        f.write(f"-Y {h} +X {w}\n".encode())
        f.write(rgbe_scanlines(px.reshape(h, w, 4), compression))


def save_png_u8(u8_rgb, path):
    """[H,W,3] uint8 device/host tensor -> PNG (generate_hdr.py:244-245 uses PIL the same way)."""
    from PIL import Image

    Image.fromarray(u8_rgb.cpu().numpy() if torch.is_tensor(u8_rgb) else u8_rgb).save(path)
