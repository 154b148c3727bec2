"""Writes a randomly initialised CLIP vision encoder directory in the Hugging Face layout (config.json, model.safetensors,
preprocessor_config.json) - what `--image_encoder` / `load_image_encoder` read - and, with --adapter, a synthetic IP-Adapter checkpoint
for the tiny SD / XL UNet configs whose projection takes that encoder's embedding (--plus: whose Resampler takes its hidden states).  For trying the image-prompt path where no real
checkpoint is at hand; the pictures that come out mean nothing.

  python tools/make_image_encoder.py OUT_DIR [--hidden 160 --heads 2 --layers 3 --mlp 320 --image 56 --patch 14 --proj 48 --act quick_gelu]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def random_state_dict(cfg, seed=0, device="cpu", dtype=torch.float32):
    """Random tensors under the transformers key names: matrices N(0, 1 / fan_in) x 3, LayerNorm weights near 1, the rest small."""
    from rich_text_to_image_amd.clip_vision_encoder import empty_state_dict
    g = torch.Generator(device=device).manual_seed(seed)
    sd = {}
    for k, z in empty_state_dict(cfg).items():
        r = torch.randn(z.shape, generator=g, device=device, dtype=dtype)
        if "norm" in k and k.endswith(".weight"):
            sd[k] = 1 + 0.1 * r
        elif z.dim() >= 2 and "position" not in k:
            sd[k] = r * (3.0 * (z.numel() // z.shape[0]) ** -0.5)
        else:
            sd[k] = 0.1 * r
    return sd


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("out")
    ap.add_argument("--hidden", type=int, default=160); ap.add_argument("--heads", type=int, default=2)
    ap.add_argument("--layers", type=int, default=3); ap.add_argument("--mlp", type=int, default=320)
    ap.add_argument("--image", type=int, default=56); ap.add_argument("--patch", type=int, default=14)
    ap.add_argument("--proj", type=int, default=48); ap.add_argument("--act", default="quick_gelu", choices=["quick_gelu", "gelu"])
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--adapter", default=None, metavar="FILE", help="also write a synthetic IP-Adapter (.bin) for --unet whose E is --proj")
    ap.add_argument("--plus", action="store_true", help="with --adapter: a \"plus\" adapter - a Resampler over the encoder's hidden states (E = --hidden, "
                                                        "dim_head 64, 2 heads, 2 layers, 4 tokens) in place of the linear projection")
    ap.add_argument("--unet", default="tiny_sd", choices=["tiny_sd", "tiny_xl"])
    a = ap.parse_args()
    from rich_text_to_image_amd.clip_vision_encoder import CLIP_MEAN, CLIP_STD, check_config
    from safetensors.torch import save_file
    cfg = dict(model_type="clip_vision_model", hidden_size=a.hidden, num_attention_heads=a.heads, num_hidden_layers=a.layers, intermediate_size=a.mlp,
               hidden_act=a.act, image_size=a.image, patch_size=a.patch, projection_dim=a.proj, layer_norm_eps=1e-5, num_channels=3)
    check_config(cfg)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "config.json"), "w") as f:
        json.dump(cfg, f, indent=1)
    with open(os.path.join(a.out, "preprocessor_config.json"), "w") as f:
        json.dump(dict(crop_size={"height": a.image, "width": a.image}, size={"shortest_edge": a.image}, image_mean=list(CLIP_MEAN),
                       image_std=list(CLIP_STD), do_center_crop=True, do_normalize=True, do_resize=True, resample=3), f, indent=1)
    save_file(random_state_dict(cfg, a.seed), os.path.join(a.out, "model.safetensors"))
    print(f"wrote {a.out}: {sum(v.numel() for v in random_state_dict(cfg, a.seed).values())} parameters, {(a.image // a.patch) ** 2 + 1} tokens per image")
    if a.adapter:
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
        import ip_adapter_ref as R
        from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict as unet_sd
        ucfg = TINY_SD_CONFIG if a.unet == "tiny_sd" else TINY_XL_CONFIG
        if a.plus:
            import resampler_ref as RS
            ck = RS.synthetic_plus_checkpoint(ucfg, unet_sd(ucfg, seed=3), E=a.hidden, dim=64, dim_head=64, heads=2, T=4, depth=2)[0]
        else:
            ck, _ = R.synthetic_checkpoint(ucfg, unet_sd(ucfg, seed=3), T=4, E=a.proj)
        torch.save(ck, a.adapter)
        print(f"wrote {a.adapter}: synthetic IP-Adapter for the {a.unet} UNet, T = 4, E = {a.hidden if a.plus else a.proj}"
              + (" (plus: a Resampler, dim_head 64)" if a.plus else ""))


if __name__ == "__main__":
    main()
