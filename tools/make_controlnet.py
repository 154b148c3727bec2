"""Writes a synthetic ControlNet checkpoint (diffusers' ControlNetModel key layout, .bin or .safetensors) for the tiny SD / XL UNet
configs - what `--controlnet` / `load_controlnet` read.  The zero convolutions are NOT zero (an untrained ControlNet's are, and would
steer nothing).  For trying the control path where no real checkpoint is at hand; the pictures that come out mean nothing.

  python tools/make_controlnet.py OUT_FILE [--unet tiny_sd|tiny_xl] [--embed 16 32 32 64] [--seed 0]"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def make_controlnet(unet, out, embed=(16, 32, 32, 64), seed=0, zero_gain=1.0):
    """Keys and shapes from the engine's own weight table (controlnet.expected_weights); matrices N(0, 1 / fan_in), norm weights near 1,
    biases small, zero convolutions N(0, zero_gain^2 / fan_in)."""
    from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG
    from rich_text_to_image_amd.controlnet import expected_weights
    cfg = {"tiny_sd": TINY_SD_CONFIG, "tiny_xl": TINY_XL_CONFIG}[unet]
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in expected_weights(cfg, embed).items():
        r = torch.randn(tuple(shape), generator=g)
        zero_conv = name.startswith(("controlnet_down_blocks.", "controlnet_mid_block."))
        if name.endswith(".weight") and len(shape) >= 2:
            sd[name] = r * ((zero_gain if zero_conv else 1.0) / math.sqrt(math.prod(shape[1:])))
        elif name.endswith(".weight"):
            sd[name] = 1.0 + 0.1 * r
        else:
            sd[name] = 0.05 * r
    if out.endswith(".safetensors"):
        from safetensors.torch import save_file
        save_file(sd, out)
    else:
        torch.save(sd, out)
    return sd


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--unet", default="tiny_sd", choices=["tiny_sd", "tiny_xl"])
    ap.add_argument("--embed", type=int, nargs=4, default=(16, 32, 32, 64), metavar="CH", help="the hint embedder's four stage widths (multiples of 8)")
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    sd = make_controlnet(a.unet, a.out, tuple(a.embed), a.seed)
    print(f"wrote {a.out}: {len(sd)} tensors, {sum(v.numel() for v in sd.values())} parameters, for the {a.unet} UNet")


if __name__ == "__main__":
    main()
