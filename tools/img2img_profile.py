"""One colour-guided image-start run of RegionDiffusionXL at the SDXL shape (128 x 128 latents, random weights), meant to be run under
`rocprofv3 --kernel-trace --stats --output-format csv -- python tools/img2img_profile.py`: the trace then holds source_blend_kernel next
to step_epilogue_kernel<STEP_EULER>, background_blend_kernel and noise_latents_kernel (profiles/img2img_kernel_stats.txt).  R = 2 regions,
`--steps` x `--strength` iterations, colour guidance on every step, self-attention injection and the background blend on, every pixel of
the left half pinned."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--strength", type=float, default=0.6)
    a = p.parse_args()
    from oracle.vae import SDXL_VAE_CONFIG, random_vae_state_dict
    from rich_text_to_image_amd.engine import VaeDecoder
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    hw, R = 128, 2
    g = torch.Generator().manual_seed(0)
    vae = VaeDecoder(SDXL_VAE_CONFIG, hw, hw, device=0, state_dict=random_vae_state_dict(SDXL_VAE_CONFIG, seed=1), precise=True)
    m = RegionDiffusionXL(device=0, unet_state_dict="random0", vae=vae)
    emb = torch.randn(R + 1, 77, 2048, generator=g)
    pooled = torch.randn(R + 1, 1280, generator=g)
    mk = torch.softmax(torch.randn(R, 1, hw, hw, generator=g) * 2, 0).repeat(1, 4, 1, 1)
    m.masks = [mk[r:r + 1] for r in range(R)]
    tfd = {"word_pos": torch.tensor([2]), "font_size": torch.tensor([3.0]), "target_RGB": [torch.rand(1, 3, 1, 1, generator=g)],
           "guidance_start_step": 999, "color_guidance_weight": 0.5,
           "color_obj_atten": [torch.rand(1, 1, 8 * hw, 8 * hw, generator=g).repeat(1, 4, 1, 1)],
           "color_obj_atten_all": torch.rand(1, 4, hw, hw, generator=g)}
    x0 = 0.8 * torch.randn(1, 4, hw, hw, generator=g)
    noise = torch.randn(1, 4, hw, hw, generator=g)
    keep = torch.zeros(hw, hw)
    keep[:, :hw // 2] = 1.0
    out = m.sample(prompt=None, height=8 * hw, width=8 * hw, num_inference_steps=a.steps, guidance_scale=5.0, prompt_embeds=emb[1:],
                   negative_prompt_embeds=emb[:1], pooled_prompt_embeds=pooled[1:], negative_pooled_prompt_embeds=pooled[:1],
                   output_type="latent", run_rich_text=True, text_format_dict=tfd, use_guidance=True, inject_selfattn=0.8,
                   inject_background=0.5, image=x0, strength=a.strength, noise=noise, keep_source=keep).images
    torch.cuda.synchronize()
    n = len(m.scheduler.timesteps)
    pinned = torch.equal(out[..., :hw // 2].cpu(), x0[..., :hw // 2])
    print(f"img2img_profile: {n} iterations, finite {bool(torch.isfinite(out).all())}, pinned half returned bit-exact {pinned}")
    assert pinned


if __name__ == "__main__":
    main()
