"""The yardstick for latent sizes that are not multiples of 2 ** (levels - 1): the oracle UNet's forward with the up loop written
out, where a block with an upsampler upsamples to the spatial size of the skip tensor it meets next (diffusers: ``upsample_size
= down_block_res_samples[-1].shape[2:]`` -> ``Upsample2D`` does ``F.interpolate(x, size=that, mode="nearest")`` instead of
``scale_factor=2``).  Built from the oracle's own modules (oracle/unet.py knows only ``scale_factor=2.0``); on a size divisible by
8 it equals the stock oracle forward bit for bit (tests/test_anysize_cpu.py).  Shared by the CPU and GPU any-size tests."""
import types

import torch
import torch.nn.functional as F

from oracle.unet import timestep_embedding


def anysize_forward(self, sample, timestep, encoder_hidden_states=None, timestep_cond=None, cross_attention_kwargs=None,
                    added_cond_kwargs=None, return_dict=False):
    if not torch.is_tensor(timestep):
        timestep = torch.tensor([timestep], dtype=torch.float32, device=sample.device)
    t = timestep.reshape(-1).to(sample.device).expand(sample.shape[0])
    temb = timestep_embedding(t, self.config.block_out_channels[0], self.config.flip_sin_to_cos, self.config.freq_shift)
    temb = self.time_embedding(temb.to(sample.dtype))
    if self.config.addition_embed_type == "text_time":
        text_embeds, time_ids = added_cond_kwargs["text_embeds"], added_cond_kwargs["time_ids"]
        te = timestep_embedding(time_ids.flatten(), self.config.addition_time_embed_dim, self.config.flip_sin_to_cos, self.config.freq_shift)
        te = te.reshape(text_embeds.shape[0], -1)
        temb = temb + self.add_embedding(torch.cat([text_embeds, te], dim=-1).to(sample.dtype))
    x = self.conv_in(sample)
    skips = [x]
    for blk in self.down_blocks:
        x, outs = blk(x, temb, encoder_hidden_states)
        skips.extend(outs)
    x = self.mid_block(x, temb, encoder_hidden_states)
    for blk in self.up_blocks:
        size = skips[-(len(blk.resnets) + 1)].shape[-2:] if blk.has_up else None  # taken before the pops
        for i, r in enumerate(blk.resnets):
            x = r(torch.cat([x, skips.pop()], dim=1), temb)
            if blk.has_attn:
                x = blk.attentions[i](x, encoder_hidden_states)
        if blk.has_up:
            x = blk.upsamplers[0].conv(F.interpolate(x, size=tuple(size), mode="nearest"))
    x = self.conv_out(F.silu(self.conv_norm_out(x)))
    return (x,)


def bind(oracle_unet):
    """Make ``oracle_unet(...)`` run the any-size forward (so oracle.pipelines' loops run unchanged); returns the model."""
    oracle_unet.forward = types.MethodType(anysize_forward, oracle_unet)
    return oracle_unet
