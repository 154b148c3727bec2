"""Drop-in for `models/region_diffusion.py:RegionDiffusion` (SD-v1.5, PNDM/PLMS) with the denoising hot path
on the HIP engine.  Same method names / argument meaning / attributes as the reference."""
import torch

from . import denoise_loop, img2img
from .engine import SD15_CONFIG
from .freeu import FreeUMixin
from .controlnet import ControlNetMixin
from .pag import PagMixin, twin_count
from .regional_lora import RegionalLoraMixin
from .ip_adapter import IPAdapterMixin
from .schedulers import DPMSolverTables, PNDMTables, engine_prediction
from .unet import HipUNet2DConditionModel


class RegionDiffusion(FreeUMixin, IPAdapterMixin, ControlNetMixin, RegionalLoraMixin, PagMixin):
    def __init__(self, device=0, unet_state_dict=None, config=None, vae=None, tokenizer=None, text_encoder=None, load_path=None,
                 latent_hw=None, vae_dir=None, vae_encoder=None, scheduler=None, max_prompt_chunks=1, guidance_rescale=0.0,
                 prediction_type=None):
        """`guidance_rescale` (pipeline attribute, default 0): the CFG rescale (rescale_noise_cfg of the SDXL reference pipeline) of every
        sampling call whose own `guidance_rescale` is 0.  `prediction_type` ('epsilon' / 'v_prediction'; None = what `load_path`'s
        scheduler/scheduler_config.json says, else epsilon): the parameterisation of the default scheduler; a scheduler passed in or
        assigned later carries its own `prediction_type`.
        `RegionDiffusion(device)` as sample.py:26-27 calls it: the reference loads runwayml/stable-diffusion-v1-5 there
        (rd.py:26-33); here the same id is resolved to a local diffusers-layout directory (checkpoint.resolve_checkpoint:
        `load_path` directory / $RTDIFF_SD_PATH / the Hugging Face hub cache) and UNet, VAE decoder, tokenizer and text encoder are
        loaded from it.  Callers that hold the weights already pass `unet_state_dict` (reference key names) and, optionally, VAE /
        CLIP objects with the diffusers / transformers call surface (`.decode(z).sample`, tokenizer(...), text_encoder(ids)[0]).
        `vae_encoder` (engine.VaeEncoder) serves encode_imgs; without it encode_imgs builds one from the AutoencoderKL weights in
        `vae_dir` on its first call.  `scheduler`: PNDMTables (the default, rd.py:35-36) or DPMSolverTables (either algorithm); assigning
        `self.scheduler` later works the same way (the diffusers idiom).  `max_prompt_chunks` (1, 2 or 3; also an argument of
        prompt_to_img / produce_attn_maps / get_text_embeds*): prompts of up to that many 75-token windows are encoded window by window
        and attended over 77 keys per window; 1 (default) cuts a prompt at 77 tokens as the reference does."""
        from .clip_tokenizer import check_max_prompt_chunks
        self.max_prompt_chunks = check_max_prompt_chunks(max_prompt_chunks)
        self.device_index = device if isinstance(device, int) else (torch.device(device).index or 0)
        self.device = torch.device(f"cuda:{self.device_index}")
        self.num_train_timesteps = 1000
        if unet_state_dict is None:
            from .checkpoint import load_components, resolve_checkpoint
            comp = load_components(resolve_checkpoint(load_path, "SD"), "SD", self.device_index, latent_hw)
            unet_state_dict, config = comp["unet_state_dict"], config or comp["config"]
            vae, tokenizer, text_encoder = vae or comp["vae"], tokenizer or comp["tokenizer"], text_encoder or comp["text_encoder"]
            vae_dir = vae_dir or comp["vae_dir"]
            prediction_type = prediction_type or comp.get("prediction_type")
        self.guidance_rescale = float(guidance_rescale)
        self.vae, self.tokenizer, self.text_encoder = vae, tokenizer, text_encoder
        self.vae_dir, self.vae_encoder = vae_dir, vae_encoder
        self._lazy_encoder = None                  # (encoder built from vae_dir, or None: no encoder weights there)
        self.unet = HipUNet2DConditionModel(config or SD15_CONFIG, unet_state_dict, self.device_index)
        self.scheduler = scheduler if scheduler is not None else PNDMTables(self.num_train_timesteps, prediction_type=prediction_type or 'epsilon')          # rd.py:35-36
        self.alphas_cumprod = torch.tensor(self.scheduler.alphas_cumprod)
        self.masks = []
        self.attention_maps = None
        self.selfattn_maps = None
        self.crossattn_maps = None
        self.n_maps = None
        self.color_loss = torch.nn.functional.mse_loss

    def _chunks(self, max_prompt_chunks):
        from .clip_tokenizer import check_max_prompt_chunks
        return check_max_prompt_chunks(self.max_prompt_chunks if max_prompt_chunks is None else max_prompt_chunks)

    def _embed_chunked(self, texts, max_chunks):
        """texts -> (embeddings [P, 77 c_max, D], key counts [P]): every 77-id window through the text encoder as a row of its own."""
        from .clip_tokenizer import encode_text_chunked

        def rows(_, ids):
            with torch.no_grad():
                return self.text_encoder(ids.to(self.device))[0], None
        emb, counts, _ = encode_text_chunked([self.tokenizer], rows, texts, max_chunks)
        return emb, counts

    # rd.py:49-84.  max_prompt_chunks > 1: (embeddings [1 + P, 77 c_max, D] zero-padded behind every prompt's own keys, key counts)
    def get_text_embeds(self, prompt, negative_prompt, max_prompt_chunks=None):
        if self.tokenizer is None or self.text_encoder is None:
            raise RuntimeError("RegionDiffusion.get_text_embeds needs a CLIP tokenizer + text encoder (not available offline)")
        chunks = self._chunks(max_prompt_chunks)
        if chunks > 1:
            prompt = [prompt] if isinstance(prompt, str) else list(prompt)
            negative_prompt = [negative_prompt] if isinstance(negative_prompt, str) else list(negative_prompt)
            return self._embed_chunked(negative_prompt + prompt, chunks)
        ti = self.tokenizer(prompt, padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                            return_tensors="pt")
        with torch.no_grad():
            te = self.text_encoder(ti.input_ids.to(self.device))[0]
        ui = self.tokenizer(negative_prompt, padding="max_length", max_length=self.tokenizer.model_max_length, return_tensors="pt")
        with torch.no_grad():
            ue = self.text_encoder(ui.input_ids.to(self.device))[0]
        return torch.cat([ue, te])

    # rd.py:72-84.  max_prompt_chunks > 1: (list of [1, 77 c_p, D] embeddings, key counts)
    def get_text_embeds_list(self, prompts, max_prompt_chunks=None):
        if self.tokenizer is None or self.text_encoder is None:
            raise RuntimeError("RegionDiffusion.get_text_embeds_list needs a CLIP tokenizer + text encoder (not available offline)")
        chunks = self._chunks(max_prompt_chunks)
        if chunks > 1:
            emb, counts = self._embed_chunked(list(prompts), chunks)
            return [emb[p:p + 1, :c] for p, c in enumerate(counts)], counts
        out = []
        for prompt in prompts:
            ti = self.tokenizer([prompt], padding="max_length", max_length=self.tokenizer.model_max_length, truncation=True,
                                return_tensors="pt")
            with torch.no_grad():
                out.append(self.text_encoder(ti.input_ids.to(self.device))[0])
        return out

    # rd.py:238-246 (denoise_loop.encode_imgs: `.encode` of the VAE object, `vae_encoder`, or an encoder built from `vae_dir`)
    def encode_imgs(self, imgs):
        return denoise_loop.encode_imgs(self, imgs, "SD", 0.18215, getattr(self.vae, "precise", False))

    def _schedule_kind(self):
        """The engine's schedule kind of self.scheduler: SD-v1.5 runs PNDM (the reference) or DPM-Solver++, nothing else."""
        if not isinstance(self.scheduler, (PNDMTables, DPMSolverTables)):
            raise ValueError(f"RegionDiffusion: scheduler must be PNDMTables or DPMSolverTables, got {type(self.scheduler).__name__}")
        return self.scheduler.kind

    # rd.py:86-174
    def produce_latents(self, text_embeddings, height=512, width=512, num_inference_steps=50, guidance_scale=7.5,
                        latents=None, use_guidance=False, text_format_dict={}, inject_selfattn=0, inject_background=0,
                        elide_dead_forwards=False, image=None, strength=0.8, noise=None, keep_source=None, key_counts=None,
                        noise_seed=None, guidance_rescale=0.0):
        """`guidance_rescale`: CFG rescale of the composed prediction (and, with its own factor, of the reference pair); 0 = the
        pipeline attribute `guidance_rescale`; applied only when guidance_scale > 1.
        `noise_seed`: seed of the per-step noise of a stochastic scheduler (DPMSolverTables(algorithm='sde-dpmsolver++')); None = 0;
        a deterministic scheduler ignores it.  The plain pass of the same seed sees the same noise at every step.
        `image` / `strength` / `noise` / `keep_source` (img2img.py): start from an existing image instead of noise, run the last
        `strength` of the schedule and pin the pixels of `keep_source` to the image at every step.  image=None: the reference's
        behaviour, the other three are not read.  `text_embeddings`: [P, 77, D] as the reference passes them, or - long prompts - what
        get_text_embeds(max_prompt_chunks > 1) returns: [P, 77 c, D] with `key_counts` (or the pair as one argument)."""
        if isinstance(text_embeddings, tuple):
            text_embeddings, key_counts = text_embeddings
        img2img.check_start(image, latents)
        if image is not None:
            latents = self._start_noise(image, noise)
        elif latents is None:
            latents = torch.randn((1, self.unet.in_channels, height // 8, width // 8), device=self.device)
        if use_guidance and not hasattr(self.vae, "color_guidance"):
            raise RuntimeError("use_guidance=True needs a rich_text_to_image_amd.engine.VaeDecoder as `vae` (rd.py:151-168)")
        n_styles = text_embeddings.shape[0] - 1
        assert n_styles == len(self.masks)                                  # rd.py:97
        h, w = latents.shape[2], latents.shape[3]
        n_prompts = text_embeddings.shape[0]
        ip_slots = self.image_prompt_slots(n_prompts, True)               # (a region index beyond the request's regions raises here, before any launch)
        cn_scales = self.control_scales(n_prompts, True)                  # (likewise)
        lora_scales = self.lora_slot_scales(n_prompts, True)              # (likewise)
        pag_scales = self.pag_slot_scales(n_prompts, True, guidance_scale, engine_prediction(self.scheduler, guidance_scale, guidance_rescale, self.guidance_rescale)[1])      # (likewise, and the refused combinations)
        eng = self.unet.engine(h, w, streams=n_prompts + 2 + twin_count(pag_scales, True), prompts=n_prompts, keys=max(key_counts) if key_counts else text_embeddings.shape[1])
        self.scheduler.set_timesteps(num_inference_steps, strength if image is not None else 1.0)
        keep = None
        if image is not None:
            x0 = img2img.source_latents(self, image)
            keep = img2img.keep_mask(self, keep_source, h, w)
        eng.set_prompts(text_embeddings.to(self.device), key_counts=key_counts)
        self.apply_image_prompts(eng, ip_slots, n_prompts)
        self.apply_control(eng, cn_scales, h, w)
        self.apply_lora_scales(eng, lora_scales)
        self.apply_pag(eng, pag_scales)
        eng.set_masks([m.to(self.device) for m in self.masks])
        tfd = text_format_dict or {}
        eng.set_fontsize(tfd.get("word_pos"), tfd.get("font_size"))
        eng.set_schedule(self._schedule_kind(), self.scheduler.timesteps.tolist(), self.scheduler.table(), num_inference_steps)
        eng.set_noise_seed(noise_seed)
        eng.set_prediction(*engine_prediction(self.scheduler, guidance_scale, guidance_rescale, self.guidance_rescale))
        self.apply_freeu(eng)
        levels = denoise_loop.start(self, eng, latents, None if image is None else x0, keep)
        denoise_loop.rich_steps(self, eng, h, w, guidance_scale, inject_selfattn, inject_background, xl=False, elide=elide_dead_forwards,
                                use_guidance=use_guidance, tfd=tfd, guidance_vae=self.vae, keep=keep, levels=levels)
        return denoise_loop.finish(eng, h, w, image is not None)

    # image start (img2img.py): the noise is drawn where `latents` is drawn, so the plain and the rich pass of one seed share their start
    def _start_noise(self, image, noise):
        h, w = img2img.latent_shape(image)
        if noise is None:
            noise = torch.randn((1, self.unet.in_channels, h, w), device=self.device)
        if tuple(noise.shape) != (1, 4, h, w):
            raise ValueError(f"noise: expected {(1, 4, h, w)}, got {tuple(noise.shape)}")
        return noise

    def predict_x0(self, x_t, eps_t, t):                                    # rd.py:176-178
        a = self.alphas_cumprod[int(t)].to(x_t.device)
        return (x_t - eps_t * torch.sqrt(1 - a)) / torch.sqrt(a)

    # rd.py:180-225 (plain pass; attention-map capture = SURVEY 8a row a10, next)
    def produce_attn_maps(self, prompts, negative_prompts='', height=512, width=512, num_inference_steps=50,
                          guidance_scale=7.5, latents=None, image=None, strength=0.8, noise=None, max_prompt_chunks=None, noise_seed=None,
                          guidance_rescale=0.0):
        if isinstance(prompts, str):
            prompts = [prompts]
        if isinstance(negative_prompts, str):
            negative_prompts = [negative_prompts]
        emb = self.get_text_embeds(prompts, negative_prompts, max_prompt_chunks)
        lat = self.plain_latents(emb, height, width, num_inference_steps, guidance_scale, latents, image=image, strength=strength, noise=noise,
                                 noise_seed=noise_seed, guidance_rescale=guidance_rescale)
        return self.latents_to_uint8(lat)

    def plain_latents(self, text_embeddings, height=512, width=512, num_inference_steps=50, guidance_scale=7.5, latents=None,
                      image=None, strength=0.8, noise=None, key_counts=None, noise_seed=None, guidance_rescale=0.0):
        if isinstance(text_embeddings, tuple):                              # get_text_embeds(max_prompt_chunks > 1): (embeddings, key counts)
            text_embeddings, key_counts = text_embeddings
        img2img.check_start(image, latents)
        if image is not None:
            latents = self._start_noise(image, noise)
        elif latents is None:
            latents = torch.randn((1, self.unet.in_channels, height // 8, width // 8), device=self.device)
        h, w = latents.shape[2], latents.shape[3]
        n_prompts = text_embeddings.shape[0]
        ip_slots = self.image_prompt_slots(n_prompts, False)
        cn_scales = self.control_scales(n_prompts, False)
        lora_scales = self.lora_slot_scales(n_prompts, False)
        pag_scales = self.pag_slot_scales(n_prompts, False, guidance_scale, engine_prediction(self.scheduler, guidance_scale, guidance_rescale, self.guidance_rescale)[1])
        eng = self.unet.engine(h, w, streams=n_prompts + 2 + twin_count(pag_scales, False), prompts=n_prompts, keys=max(key_counts) if key_counts else text_embeddings.shape[1])
        self.scheduler.set_timesteps(num_inference_steps, strength if image is not None else 1.0)
        if image is not None:
            img2img.check_tokenmap_iterations(getattr(self, "_tokenmap_hooks", False), len(self.scheduler.timesteps))
        eng.set_prompts(text_embeddings.to(self.device), key_counts=key_counts)
        self.apply_image_prompts(eng, ip_slots, n_prompts)
        self.apply_control(eng, cn_scales, h, w)
        self.apply_lora_scales(eng, lora_scales)
        self.apply_pag(eng, pag_scales)
        eng.set_schedule(self._schedule_kind(), self.scheduler.timesteps.tolist(), self.scheduler.table(), num_inference_steps)
        eng.set_noise_seed(noise_seed)
        eng.set_prediction(*engine_prediction(self.scheduler, guidance_scale, guidance_rescale, self.guidance_rescale))
        self.apply_freeu(eng)
        denoise_loop.start(self, eng, latents, None if image is None else img2img.source_latents(self, image))
        denoise_loop.plain_steps(self, eng, guidance_scale)
        return denoise_loop.finish(eng, h, w, image is not None)

    def decode_latents(self, latents):                                      # rd.py:227-236
        if self.vae is None:
            raise RuntimeError("no VAE bound: pass `vae=` (engine.VaeDecoder or an object with .decode(z).sample)")
        latents = 1 / 0.18215 * latents
        with torch.no_grad():
            imgs = self.vae.decode(latents)
            imgs = getattr(imgs, "sample", imgs)               # diffusers-style object or the engine's VaeDecoder tensor
        return (imgs / 2 + 0.5).clamp(0, 1)

    def latents_to_uint8(self, latents):
        imgs = self.decode_latents(latents)
        imgs = imgs.detach().cpu().permute(0, 2, 3, 1).numpy()
        return (imgs * 255).round().astype('uint8')

    # rd.py:248-273
    def prompt_to_img(self, prompts, negative_prompts='', height=512, width=512, num_inference_steps=50, guidance_scale=7.5,
                      latents=None, text_format_dict={}, use_guidance=False, inject_selfattn=0, inject_background=0,
                      image=None, strength=0.8, noise=None, keep_source=None, max_prompt_chunks=None, noise_seed=None, guidance_rescale=0.0):
        if isinstance(prompts, str):
            prompts = [prompts]
        if isinstance(negative_prompts, str):
            negative_prompts = [negative_prompts]
        text_embeds = self.get_text_embeds(prompts, negative_prompts, max_prompt_chunks)
        latents = self.produce_latents(text_embeds, height=height, width=width, latents=latents,
                                       num_inference_steps=num_inference_steps, guidance_scale=guidance_scale,
                                       use_guidance=use_guidance, text_format_dict=text_format_dict,
                                       inject_selfattn=inject_selfattn, inject_background=inject_background,
                                       image=image, strength=strength, noise=noise, keep_source=keep_source, noise_seed=noise_seed,
                                       guidance_rescale=guidance_rescale)
        return self.latents_to_uint8(latents)

    # hook surface of the reference (rd.py:397-443): token-map capture is the "next" row f1
    def reset_attention_maps(self):                                         # rd.py:275-283
        for maps in (self.selfattn_maps, self.crossattn_maps):
            for key in (maps or {}):
                maps[key] = []

    def register_tokenmap_hooks(self):
        """rd.py:397-443: record head-averaged maps of the conditional half during produce_attn_maps / plain_latents.
        Recording happens on the GPU (rt_attn_store_*); the dicts are filled after each plain pass."""
        import collections
        self._tokenmap_hooks = True
        self.selfattn_maps = collections.defaultdict(list)
        self.crossattn_maps = collections.defaultdict(list)
        self.n_maps = collections.defaultdict(list)

    def remove_tokenmap_hooks(self):
        self._tokenmap_hooks = False
        self.selfattn_maps = self.crossattn_maps = self.n_maps = None

    def _store_begin(self, eng):
        from .attention_utils import CrossAttentionLayers, SelfAttentionLayers
        self._recorded = []
        for name, max_tokens, _ in eng.attn_modules():
            if name in SelfAttentionLayers and max_tokens <= 1024:
                eng.attn_store_enable(name, 2)       # rd.py:423: tests `name in crossattn_maps` => overwritten each step
                self._recorded.append(name)
            elif name in CrossAttentionLayers:
                eng.attn_store_enable(name, 1)
                self._recorded.append(name)
            else:
                eng.attn_store_enable(name, 0)
        eng.attn_store_reset()

    def _store_end(self, eng, n_calls):
        for name, _, _ in eng.attn_modules():
            self.n_maps[name] = (self.n_maps[name] if name in self.n_maps else 0) + n_calls
        for name in self._recorded:
            n, m = eng.attn_store_read(name)
            if m is None:
                continue
            tgt = self.crossattn_maps if name.endswith("attn2") else self.selfattn_maps
            if name.endswith("attn2") and name in tgt and not isinstance(tgt[name], list):
                tgt[name] = tgt[name] + m                # (on the GPU: get_token_maps averages there)
            else:
                tgt[name] = m
            eng.attn_store_enable(name, 0)
