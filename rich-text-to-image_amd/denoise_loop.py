"""What the two pipelines (region_diffusion.py, region_diffusion_sdxl.py) share once the engine holds the prompts and the schedule: the
start, the rich-text and the plain step loops, the finish, and the VAE encoder behind `encode_imgs`.  `pipe` is the pipeline object
(its scheduler, masks, device, split_image flag and token-map hooks are read), `eng` its engine."""
import torch

from .controlnet import switch_control


def start(pipe, eng, latents, x0=None, keep=None):
    """Sets the engine's start latents: `latents` as given, or - with a source x0 - a*x0 + b*latents at the scheduler's start level
    (`latents` is the noise then).  Returns the per-iteration source levels (None without a source)."""
    if x0 is None:
        eng.set_latents(latents.to(pipe.device))
        return None
    eng.set_source(x0, latents.to(pipe.device), keep)
    eng.noise_latents(*pipe.scheduler.start_level())
    return pipe.scheduler.source_levels()


def finish(eng, h, w, had_source):
    out = eng.read_latents(h, w)
    if had_source:
        eng.set_source(None)
    return out


# rd.py:99-173 / xl.py:779-872
def rich_steps(pipe, eng, h, w, guidance_scale, inject_selfattn, inject_background, *, xl, elide, use_guidance, tfd, guidance_vae,
               keep=None, levels=None, callback=None, callback_steps=1):
    split = getattr(pipe, "split_image", False)
    for i in range(len(pipe.scheduler.timesteps)):
        switch_control(pipe, eng, i)             # ControlNet (set_control's start / end): the scales go on and off between steps
        if split:
            # intra-image split (launcher.split_region_step): the ranks of the process group share THIS image's step - each runs
            # the forwards of its stream range, one exchange of the noise predictions, every rank finishes the step
            from .launcher import assert_ranks_agree, split_region_step
            if i % 10 == 0:                      # every rank must hold the same masks / latents (homogeneous ranks): fail loudly otherwise
                if i == 0:
                    assert_ranks_agree(torch.cat([m.reshape(-1).float().cpu() for m in pipe.masks]), "the region masks")
                assert_ranks_agree(eng.read_latents(h, w), f"the latents before step {i}")
            split_region_step(eng, i, guidance_scale, inject_selfattn, inject_background, xl, elide=elide, defer_blend=use_guidance)
        else:
            eng.region_step(i, guidance_scale, inject_selfattn, inject_background, xl=xl, elide=elide, defer_blend=use_guidance)
        if use_guidance:
            t = float(pipe.scheduler.timesteps[i])
            if t < tfd['guidance_start_step']:                   # rd.py:151 / xl.py:849; predict_x0 on the unscaled Euler latents (quirk 4; DPM: unscaled anyway)
                lat_ptr, eps_ptr = eng.state_ptrs()

                def guide(lat_ptr=lat_ptr, eps_ptr=eps_ptr, t=t):
                    guidance_vae.color_guidance(lat_ptr, eps_ptr, float(pipe.scheduler.alphas_cumprod[int(t)]), h, w, tfd['color_obj_atten'],
                                                tfd['target_RGB'], tfd['color_guidance_weight'], tfd['color_obj_atten_all'])
                if split:                                        # rank 0 runs the VAE pass, the others receive the updated latents
                    from .launcher import guidance_from_rank0
                    guidance_from_rank0(eng, guide, h, w)
                else:
                    guide()
            eng.background_blend()
        if keep is not None:
            eng.source_blend(*levels[i])
        if callback is not None and i % callback_steps == 0:
            callback(i, pipe.scheduler.timesteps[i], eng.read_latents(h, w))


# rd.py:200-214 / xl.py:880-905, with the token-map hooks of the pipeline around the loop
def plain_steps(pipe, eng, guidance_scale):
    n = len(pipe.scheduler.timesteps)
    hooks = getattr(pipe, "_tokenmap_hooks", False)
    if hooks:
        pipe._store_begin(eng)
    for i in range(n):
        switch_control(pipe, eng, i)
        if getattr(pipe, "split_image", False):                  # one stream per rank, the text stream's rank records the maps
            from .launcher import split_plain_step
            split_plain_step(eng, i, guidance_scale)
        else:
            eng.plain_step(i, guidance_scale)
    if hooks:
        pipe._store_end(eng, n)


# rd.py:238-246.  In order: a VAE object with `.encode` (the reference behaviour), the `vae_encoder` given to the constructor, an
# encoder built from `vae_dir` on the first call (sized to the largest image seen: rebuilt when a larger one arrives; the rich-text
# flow never encodes, so it pays nothing for this), else NotImplementedError.  The 2x - 1 and the scaling factor run in the HIP kernels.
def encode_imgs(pipe, imgs, family, scale, precise):
    if hasattr(pipe.vae, "encode"):
        imgs = 2 * imgs - 1
        return pipe.vae.encode(imgs).latent_dist.sample() * scale
    enc = pipe.vae_encoder or _encoder_from_dir(pipe, imgs.shape[-2], imgs.shape[-1], family, precise)
    if enc is None:
        raise NotImplementedError("encode_imgs needs VAE encoder weights: a VAE with `.encode`, `vae_encoder=`, or an AutoencoderKL "
                                  "directory whose weights hold `encoder.*` (this one is decoder-only)")
    return enc.encode(imgs, in_scale=2.0, in_shift=-1.0).latent_dist.sample(scale=scale)


def _encoder_from_dir(pipe, H, W, family, precise):
    if pipe.vae_dir is None:
        return None
    lat = (-(-H // 8), -(-W // 8))
    if pipe._lazy_encoder is not None:
        enc = pipe._lazy_encoder[0]
        if enc is None or (lat[0] <= enc.cfg.latent_h and lat[1] <= enc.cfg.latent_w):
            return enc
        lat = (max(lat[0], enc.cfg.latent_h), max(lat[1], enc.cfg.latent_w))
        enc.close()
    from .checkpoint import load_vae_encoder
    enc = load_vae_encoder(pipe.vae_dir, family, pipe.device_index, lat, precise=precise)
    pipe._lazy_encoder = (enc,)
    return enc
