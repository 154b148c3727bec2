"""Test helper (not collected): AutoencoderKL *encoder* + quant_conv restated in functional fp32 torch, the reference the HIP
encoder (VaeEncoder / rt_vae_encode) is pinned against.

[memory] diffusers 0.18.2 (`models/vae.py:Encoder`, `unet_2d_blocks.py:DownEncoderBlock2D / UNetMidBlock2D`, `resnet.py:Downsample2D`,
`models/vae.py:DiagonalGaussianDistribution`) is third-party code that is not on disk: this restates the published architecture from
memory, like oracle/vae.py does for the decoder, so parity against diffusers is UNPINNED.  The blocks reuse OracleVAEDecoder's
`_conv / _gn / _resnet / _attn`.
"""
import math
from collections import OrderedDict

import torch
import torch.nn.functional as F

from oracle.vae import OracleVAEDecoder


def vae_encoder_shapes(cfg):
    """State-dict names and shapes of AutoencoderKL.encoder + quant_conv."""
    s = OrderedDict()
    boc = cfg["block_out_channels"]
    lc = cfg.get("latent_channels", 4)

    def conv(n, i, o, k):
        s[n + ".weight"] = (o, i, k, k); s[n + ".bias"] = (o,)

    def norm(n, c):
        s[n + ".weight"] = (c,); s[n + ".bias"] = (c,)

    def lin(n, i, o):
        s[n + ".weight"] = (o, i); s[n + ".bias"] = (o,)

    def resnet(n, i, o):
        norm(n + ".norm1", i); conv(n + ".conv1", i, o, 3); norm(n + ".norm2", o); conv(n + ".conv2", o, o, 3)
        if i != o:
            conv(n + ".conv_shortcut", i, o, 1)
    conv("encoder.conv_in", 3, boc[0], 3)
    out_c = boc[0]
    for i, c in enumerate(boc):
        prev, out_c = out_c, c
        for j in range(cfg["layers_per_block"]):
            resnet(f"encoder.down_blocks.{i}.resnets.{j}", prev if j == 0 else out_c, out_c)
        if i != len(boc) - 1:
            conv(f"encoder.down_blocks.{i}.downsamplers.0.conv", out_c, out_c, 3)
    top = boc[-1]
    resnet("encoder.mid_block.resnets.0", top, top)
    a = "encoder.mid_block.attentions.0"
    norm(a + ".group_norm", top)
    lin(a + ".to_q", top, top); lin(a + ".to_k", top, top); lin(a + ".to_v", top, top); lin(a + ".to_out.0", top, top)
    resnet("encoder.mid_block.resnets.1", top, top)
    norm("encoder.conv_norm_out", top)
    conv("encoder.conv_out", top, 2 * lc, 3)
    conv("quant_conv", 2 * lc, 2 * lc, 1)
    return s


def random_vae_encoder_state_dict(cfg, seed=0):
    """Same init scheme as oracle.vae.random_vae_state_dict: U(-1, 1) / sqrt(fan_in) weights, norm scales 1 +- 0.1, biases +- 0.05."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in vae_encoder_shapes(cfg).items():
        if name.endswith(".weight") and len(shape) >= 2:
            fan_in = math.prod(shape[1:])
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
        elif name.endswith(".weight"):
            sd[name] = 1.0 + 0.1 * (torch.rand(shape, generator=g) * 2 - 1)
        else:
            sd[name] = 0.05 * (torch.rand(shape, generator=g) * 2 - 1)
    return sd


class OracleVAEEncoder(OracleVAEDecoder):
    """[memory] diffusers 0.18.2 AutoencoderKL.encode up to the posterior's moments (fp32, functional)."""

    def moments(self, x):
        """x [B, 3, H, W] (already 2 * imgs - 1) -> [B, 8, H/8, W/8]: mean | clamp(logvar, -30, 20)."""
        x = self._conv(x.float(), "encoder.conv_in")
        n = len(self.cfg["block_out_channels"])
        for i in range(n):
            for j in range(self.cfg["layers_per_block"]):
                x = self._resnet(x, f"encoder.down_blocks.{i}.resnets.{j}")
            if i != n - 1:                                   # Downsample2D(padding=0): zero row / column at the bottom / right only
                d = f"encoder.down_blocks.{i}.downsamplers.0.conv"
                x = F.conv2d(F.pad(x, (0, 1, 0, 1)), self.sd[d + ".weight"], self.sd[d + ".bias"], stride=2)
        x = self._resnet(x, "encoder.mid_block.resnets.0")
        x = self._attn(x, "encoder.mid_block.attentions.0")
        x = self._resnet(x, "encoder.mid_block.resnets.1")
        x = self._conv(F.silu(self._gn(x, "encoder.conv_norm_out")), "encoder.conv_out")
        m = self._conv(x, "quant_conv", padding=0)
        mean, logvar = m.chunk(2, dim=1)
        return torch.cat([mean, logvar.clamp(-30.0, 20.0)], dim=1)
