"""Drop-in for `models/region_diffusion_sdxl.py:RegionDiffusionXL` (SDXL, Euler) with the denoising hot path on
the HIP engine.  `sample()` keeps the reference's signature (xl.py:556-587)."""
import types

import torch

from . import denoise_loop, img2img
from .engine import SDXL_CONFIG
from .freeu import FreeUMixin
from .controlnet import ControlNetMixin
from .pag import PagMixin, twin_count
from .regional_lora import RegionalLoraMixin
from .ip_adapter import IPAdapterMixin
from .schedulers import DPMSolverTables, EulerAncestralTables, EulerTables, engine_prediction
from .unet import HipUNet2DConditionModel


class StableDiffusionXLPipelineOutput(dict):
    def __init__(self, images):
        super().__init__(images=images)
        self.images = images


class RegionDiffusionXL(FreeUMixin, IPAdapterMixin, ControlNetMixin, RegionalLoraMixin, PagMixin):
    def __init__(self, load_path=None, device=0, unet_state_dict=None, config=None, vae=None, text_encoders=None,
                 vae_scaling_factor=0.13025, tokenizer=None, latent_hw=None, scheduler=None, vae_dir=None, vae_encoder=None,
                 max_prompt_chunks=1, guidance_rescale=0.0, prediction_type=None):
        """`guidance_rescale` (pipeline attribute, default 0): the CFG rescale of both passes when the call's own `guidance_rescale` is 0 -
        the only way to rescale the rich pass, whose call keyword the reference refuses (xl.py:827-830).  `prediction_type` ('epsilon' /
        'v_prediction'; None = what `load_path`'s scheduler/scheduler_config.json says, else epsilon): the parameterisation of the
        default scheduler; a scheduler passed in or assigned later carries its own `prediction_type`.
        `RegionDiffusionXL(load_path="stabilityai/stable-diffusion-xl-base-1.0")` as sample.py:28-30 calls it (xl.py:105-120
        loads every component from `load_path`): a diffusers-layout directory, or a hub id resolved to one without a network
        (checkpoint.resolve_checkpoint: $RTDIFF_SDXL_PATH for the default id, then the Hugging Face hub cache).  Callers that hold
        the weights pass `unet_state_dict` (+ optional vae / text_encoders / tokenizer) and `load_path` is not read.
        `scheduler`: EulerTables (the default, xl.py:120), EulerAncestralTables or DPMSolverTables (either algorithm); assigning `self.scheduler` later works the same way.
        `vae_encoder` (engine.VaeEncoder) serves encode_imgs; without it encode_imgs builds one from the AutoencoderKL weights in
        `vae_dir` on its first call."""
        self.device_index = device if isinstance(device, int) else (torch.device(device).index or 0)
        self.device = torch.device(f"cuda:{self.device_index}")
        self.device_type = "cuda"
        if unet_state_dict is None:
            from .checkpoint import load_components, resolve_checkpoint
            comp = load_components(resolve_checkpoint(load_path, "SDXL"), "SDXL", self.device_index, latent_hw)
            unet_state_dict, config = comp["unet_state_dict"], config or comp["config"]
            vae, text_encoders, tokenizer = vae or comp["vae"], text_encoders or comp["text_encoders"], tokenizer or comp["tokenizer"]
            vae_scaling_factor = comp["vae_scaling_factor"]
            vae_dir = vae_dir or comp.get("vae_dir")
            prediction_type = prediction_type or comp.get("prediction_type")
        self.guidance_rescale = float(guidance_rescale)
        self.unet = HipUNet2DConditionModel(config or SDXL_CONFIG, unet_state_dict, self.device_index)
        self.vae = vae
        self.vae_dir, self.vae_encoder = vae_dir, vae_encoder
        self._lazy_encoder = None                  # (encoder built from vae_dir, or None: no encoder weights there)
        # Optional (round 6): a second VaeDecoder used ONLY for the colour-guidance pass (xl.py:849-867).  The reference runs the SDXL VAE in
        # fp32 because it overflows in fp16 (xl.py:856), and `vae` (precise = three bf16 MFMA passes) follows it.  A one-pass bf16 engine has
        # fp32's range; over the 50-step guided schedule it leaves the latents where the precise engine leaves them (update-relative error
        # against the fp32 oracle 3.05e-2 -> 1.16e-2 either way, LABNOTES R6.6) for 37 instead of 80 ms per step.  None: `vae` guides too.
        self.guidance_vae = None
        self.text_encoders = text_encoders
        self.vae_scaling_factor = vae_scaling_factor
        self.vae_scale_factor = 8
        self.default_sample_size = 128
        self.scheduler = scheduler if scheduler is not None else EulerTables(prediction_type=prediction_type or 'epsilon')
        self.masks = []
        self.selfattn_maps = self.crossattn_maps = self.n_maps = None
        self.attention_maps = None                                   # xl.py:132 (only the evaluation hooks ever set it)
        self.tokenizer = tokenizer                                   # richtext_utils needs `model.tokenizer._tokenize`
        # prompts of up to this many 75-token windows are encoded window by window and attended over 77 keys per window (also an
        # argument of sample()); 1 = the reference: a prompt is cut at 77 tokens
        from .clip_tokenizer import check_max_prompt_chunks
        self.max_prompt_chunks = check_max_prompt_chunks(max_prompt_chunks)

    def reset_attention_maps(self):
        for maps in (self.selfattn_maps, self.crossattn_maps):
            for key in (maps or {}):
                maps[key] = []

    def check_inputs(self, prompt, height, width, prompt_embeds, pooled_prompt_embeds):          # xl.py:462-519
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        if prompt_embeds is not None and pooled_prompt_embeds is None:
            raise ValueError("If `prompt_embeds` are provided, `pooled_prompt_embeds` also have to be passed.")

    def _get_add_time_ids(self, original_size, crops_coords_top_left, target_size):                # xl.py:539-553
        return torch.tensor([list(original_size + crops_coords_top_left + target_size)], dtype=torch.float32)

    def encode_prompt(self, prompt, negative_prompt, max_prompt_chunks=1):
        """-> the reference's four tensors; with max_prompt_chunks > 1 also the key counts of the prompts and the negative prompts."""
        if self.text_encoders is None:
            raise RuntimeError("RegionDiffusionXL needs CLIP text encoders for string prompts (not available offline); "
                               "pass prompt_embeds / pooled_prompt_embeds instead")
        if max_prompt_chunks == 1:
            return self.text_encoders(prompt, negative_prompt)
        return self.text_encoders(prompt, negative_prompt, max_prompt_chunks=max_prompt_chunks)

    # RegionDiffusion.encode_imgs (rd.py:238-246) with the SDXL VAE: its config and scaling factor, fp32-class contractions like the
    # pipeline's decoder (xl.py:856)
    def encode_imgs(self, imgs):
        return denoise_loop.encode_imgs(self, imgs, "SDXL", self.vae_scaling_factor, True)

    def sample(self, prompt=None, prompt_2=None, height=None, width=None, num_inference_steps=50, guidance_scale=5.0,
               negative_prompt=None, negative_prompt_2=None, num_images_per_prompt=1, eta=0.0, generator=None,
               latents=None, prompt_embeds=None, negative_prompt_embeds=None, pooled_prompt_embeds=None,
               negative_pooled_prompt_embeds=None, output_type="pil", return_dict=True, callback=None, callback_steps=1,
               cross_attention_kwargs=None, guidance_rescale=0.0, original_size=None, crops_coords_top_left=(0, 0),
               target_size=None, use_guidance=False, inject_selfattn=0, inject_background=0, text_format_dict=None,
               run_rich_text=False, elide_dead_forwards=False, image=None, strength=0.8, noise=None, keep_source=None,
               max_prompt_chunks=None, prompt_key_counts=None, negative_key_counts=None, noise_seed=None):
        """`guidance_rescale` (xl.py:42-53, :903-905): the plain pass rescales the guided prediction towards the standard deviation of
        its conditional half; 0 falls back to the pipeline attribute `guidance_rescale`, which also rescales the rich pass (the mask-
        composed prediction against the composed conditional half, the reference pair against its own: xl.py:827-830's commented
        line).  With run_rich_text=True the keyword > 0 raises NotImplementedError, as in the reference.  Applied only when
        guidance_scale > 1.  A v-prediction model is run by a scheduler whose `prediction_type` is 'v_prediction'.
        `noise_seed`: seed of the per-step noise of a stochastic scheduler (EulerAncestralTables, DPMSolverTables(algorithm=
        'sde-dpmsolver++')); None = 0; a deterministic scheduler ignores it.  The plain pass (run_rich_text=False) of the same seed sees
        the same noise at every step.
        `image` / `strength` / `noise` / `keep_source` (img2img.py): start from an existing image instead of noise, run the last
        `strength` of the schedule, and (rich pass) pin the pixels of `keep_source` to the image at every step.  image=None: the
        reference's behaviour, the other three are not read.
        `max_prompt_chunks` (default: the constructor's): string prompts of up to that many 75-token windows are chunked instead of cut.
        Callers that pass `prompt_embeds` of 77 c rows say with `prompt_key_counts` / `negative_key_counts` how many rows of every
        prompt are its keys (default: all of them)."""
        from .clip_tokenizer import check_max_prompt_chunks, pad_keys
        chunks = check_max_prompt_chunks(self.max_prompt_chunks if max_prompt_chunks is None else max_prompt_chunks)
        height = height or self.default_sample_size * self.vae_scale_factor
        width = width or self.default_sample_size * self.vae_scale_factor
        original_size = original_size or (height, width)
        target_size = target_size or (height, width)
        self.check_inputs(prompt, height, width, prompt_embeds, pooled_prompt_embeds)
        if prompt_embeds is None:
            if chunks > 1:
                prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds, prompt_key_counts, \
                    negative_key_counts = self.encode_prompt(prompt, negative_prompt, chunks)
            else:
                prompt_embeds, negative_prompt_embeds, pooled_prompt_embeds, negative_pooled_prompt_embeds = \
                    self.encode_prompt(prompt, negative_prompt)
        do_cfg = guidance_scale > 1.0
        if run_rich_text and do_cfg and guidance_rescale > 0.0:
            raise NotImplementedError                                                              # xl.py:827-830
        if use_guidance and not hasattr(self.vae, "color_guidance"):
            raise RuntimeError("use_guidance=True needs a rich_text_to_image_amd.engine.VaeDecoder as `vae` (xl.py:849-867)")
        if not isinstance(self.scheduler, (EulerTables, EulerAncestralTables, DPMSolverTables)):
            raise ValueError(f"RegionDiffusionXL: scheduler must be EulerTables, EulerAncestralTables or DPMSolverTables, got {type(self.scheduler).__name__}")
        prediction = engine_prediction(self.scheduler, guidance_scale, guidance_rescale, self.guidance_rescale)
        img2img.check_start(image, latents)
        h, w = height // self.vae_scale_factor, width // self.vae_scale_factor
        if image is None:
            self.scheduler.set_timesteps(num_inference_steps)
            if latents is None:
                latents = torch.randn((1, 4, h, w), generator=generator, device=self.device if generator is None else generator.device)
            latents = latents.to(self.device).float() * self.scheduler.init_noise_sigma            # xl.py:533-536
            keep = None
        else:
            if img2img.latent_shape(image) != (h, w):
                raise ValueError(f"image {tuple(image.shape)} does not match height x width = {height} x {width}")
            self.scheduler.set_timesteps(num_inference_steps, strength)
            if noise is None:                          # drawn where `latents` is drawn: the plain and the rich pass of one seed share their start
                noise = torch.randn((1, 4, h, w), generator=generator, device=self.device if generator is None else generator.device)
            noise = noise.to(self.device).float()
            x0 = img2img.source_latents(self, image)
            keep = img2img.keep_mask(self, keep_source, h, w) if run_rich_text else None
            img2img.check_tokenmap_iterations(not run_rich_text and getattr(self, "_tokenmap_hooks", False), len(self.scheduler.timesteps))
        add_time_ids = self._get_add_time_ids(tuple(original_size), tuple(crops_coords_top_left), tuple(target_size))
        key_counts = None
        if prompt_key_counts is not None or negative_key_counts is not None or prompt_embeds.shape[1] != negative_prompt_embeds.shape[1]:
            key_counts = list(negative_key_counts or [negative_prompt_embeds.shape[1]] * negative_prompt_embeds.shape[0]) + \
                list(prompt_key_counts or [prompt_embeds.shape[1]] * prompt_embeds.shape[0])
            L = max(prompt_embeds.shape[1], negative_prompt_embeds.shape[1])
            prompt_embeds, negative_prompt_embeds = pad_keys(prompt_embeds, L), pad_keys(negative_prompt_embeds, L)
        embeds = torch.cat([negative_prompt_embeds, prompt_embeds], 0).to(self.device).float()    # xl.py:760
        pooled = torch.cat([negative_pooled_prompt_embeds, pooled_prompt_embeds], 0).to(self.device).float()
        ip_slots = self.image_prompt_slots(embeds.shape[0], run_rich_text)     # (a region index beyond the request's regions raises here, before any launch)
        cn_scales = self.control_scales(embeds.shape[0], run_rich_text)        # (likewise)
        lora_scales = self.lora_slot_scales(embeds.shape[0], run_rich_text)    # (likewise)
        pag_scales = self.pag_slot_scales(embeds.shape[0], run_rich_text, guidance_scale, prediction[1])      # (likewise, and the refused combinations)
        eng = self.unet.engine(h, w, streams=(embeds.shape[0] + 2 if run_rich_text else 2) + twin_count(pag_scales, run_rich_text), prompts=embeds.shape[0],
                               keys=max(key_counts) if key_counts else embeds.shape[1])
        eng.set_prompts(embeds, pooled, add_time_ids, key_counts=key_counts)
        self.apply_image_prompts(eng, ip_slots, embeds.shape[0])
        self.apply_control(eng, cn_scales, h, w)
        self.apply_lora_scales(eng, lora_scales)
        self.apply_pag(eng, pag_scales)
        eng.set_schedule(self.scheduler.kind, self.scheduler.timesteps.tolist(), self.scheduler.table(), num_inference_steps)
        eng.set_noise_seed(noise_seed)
        eng.set_prediction(*prediction)
        self.apply_freeu(eng)
        levels = denoise_loop.start(self, eng, latents if image is None else noise, None if image is None else x0, keep)
        if run_rich_text:
            n_styles = embeds.shape[0] - 1
            assert n_styles == len(self.masks), (n_styles, len(self.masks))
            eng.set_masks([m.to(self.device) for m in self.masks])
            tfd = text_format_dict or {}
            eng.set_fontsize(tfd.get("word_pos"), tfd.get("font_size"))
            denoise_loop.rich_steps(self, eng, h, w, guidance_scale, inject_selfattn, inject_background, xl=True, elide=elide_dead_forwards,
                                    use_guidance=use_guidance, tfd=tfd, guidance_vae=self.guidance_vae or self.vae, keep=keep, levels=levels,
                                    callback=callback, callback_steps=callback_steps)
        else:
            denoise_loop.plain_steps(self, eng, guidance_scale)
        latents = denoise_loop.finish(eng, h, w, image is not None)
        if output_type == "latent":
            return StableDiffusionXLPipelineOutput(images=latents)
        if self.vae is None:
            raise RuntimeError("no VAE bound: pass `vae=` (engine.VaeDecoder or an object with .decode(z)) or use output_type='latent'")
        image = self.vae.decode(latents / self.vae_scaling_factor)
        image = getattr(image, "sample", image)
        if output_type == "pt":
            return StableDiffusionXLPipelineOutput(images=image)
        arr = ((image / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).cpu().numpy() * 255).round().astype("uint8")    # VaeImageProcessor.postprocess
        if output_type == "np":
            return StableDiffusionXLPipelineOutput(images=arr)
        from PIL import Image
        return StableDiffusionXLPipelineOutput(images=[Image.fromarray(a) for a in arr])

    def predict_x0(self, x_t, eps_t, t):                                                           # xl.py:955-957
        a = torch.tensor(self.scheduler.alphas_cumprod)[int(t)].to(x_t.device)
        return (x_t - eps_t * torch.sqrt(1 - a)) / torch.sqrt(a)

    cross_attention_layers = None      # defaults to attention_utils.CrossAttentionLayers_XL

    def register_tokenmap_hooks(self):
        """xl.py:959-1016: every attn1 map is accumulated by the reference; only the 32x32 ones are consumed
        (attention_utils.py:243-248), so only those are recorded here (GPU side, rt_attn_store_*)."""
        import collections
        self._tokenmap_hooks = True
        self.selfattn_maps = collections.defaultdict(list)
        self.crossattn_maps = collections.defaultdict(list)
        self.n_maps = collections.defaultdict(list)

    def remove_tokenmap_hooks(self):
        self._tokenmap_hooks = False
        self.selfattn_maps = self.crossattn_maps = self.n_maps = None

    def _store_begin(self, eng):
        from .attention_utils import CrossAttentionLayers_XL
        cross = self.cross_attention_layers or CrossAttentionLayers_XL
        self._recorded = []
        for name, max_tokens, _ in eng.attn_modules():
            if name.endswith("attn1") and max_tokens <= 1024:
                eng.attn_store_enable(name, 1)
                self._recorded.append(name)
            elif name in cross:
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
            # the maps stay on the GPU (60 x 4 MB at SDXL): get_token_maps averages them there and moves ONE 1024 x 1024 affinity to the host
            tgt[name] = (tgt[name] + m) if (name in tgt and not isinstance(tgt[name], list)) else m
            eng.attn_store_enable(name, 0)
