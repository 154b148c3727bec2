"""End-to-end flow of the reference's `sample.py:17-114` on the MI355X engine:
JSON -> spans -> plain pass with on-device attention capture -> token maps (twice) -> rich-text pass.

`generate(model, param, ...)` is the body of the reference `main()` with the model passed in (checkpoints, the CLIP
tokenizer and text encoders are the caller's: none are available offline); file output is optional.
"""
import argparse
import json
import os
import sys
import time
import types

import torch
import torch.nn.functional as F

from .attention_utils import get_token_maps
from .clip_tokenizer import check_max_prompt_chunks
from .richtext_utils import (get_attention_control_input, get_gradient_guidance_input, get_region_diffusion_input, parse_json,
                             seed_everything)


def _resize_bicubic_aa(mask, height, width):
    # torchvision.transforms.functional.resize(tensor, BICUBIC, antialias=True) == this interpolate call (sample.py:83-86)
    return F.interpolate(mask, size=(height, width), mode='bicubic', antialias=True, align_corners=False)


def generate(model, param, model_type='SD', run_dir=None, color_guidance_weight=0.5, inject_selfattn=0., segment_threshold=0.3,
             num_segments=9, inject_background=0., latents=None, init_image=None, strength=0.8, keep_source=None):
    """Returns (plain_image, rich_image, timings).  `param` has the reference's keys: text_input, height, width,
    guidance_weight, steps, noise_index, negative_prompt (sample.py:135-143).
    `init_image` ([1,3,height,width] in [0,1], or [1,4,h,w] latents): both passes start from it instead of noise and run the last
    `strength` of the schedule; it is encoded once and the same latents, strength and noise go to both passes.  `keep_source`
    ("background" or a mask, img2img.py) pins those pixels of the rich pass to the image.
    `param['max_prompt_chunks']` (optional: 1, 2 or 3; default: the model's own `max_prompt_chunks`): texts of up to that many 75-token CLIP windows are chunked, in
    both passes, instead of cut at 77 tokens; a text that needs more raises ValueError.
    The request's seed (`noise_index`) is also the noise seed of a stochastic scheduler, in both passes: they see the same per-step noise.
    `param['guidance_rescale']` (optional): the CFG rescale of both passes, handed to the sampling calls as their `guidance_rescale`
    keyword; the SDXL rich pass, whose keyword the reference refuses, takes it as the pipeline attribute, set around that one call and
    restored after it.
    `param['freeu']` (optional, four numbers s1 s2 b1 b2): FreeU in both passes of THIS request - the pipeline attribute
    (enable_freeu) for the duration of the call, restored after it; absent / None: the pipeline as it is.
    `param['image_prompts']` (optional; ip_adapter.image_prompts_from_specs' result: dict(base=, regions=, negative=) of dict(file=,
    scale=)): the image prompts of THIS request on a pipeline with an IP-Adapter loaded - set for the call, restored after it; `base`
    holds in both passes, `regions` (by region number) in the rich pass; absent / None: the pipeline as it is.
    `param['region_loras']` (optional; set_lora_scales' keyword arguments, regional_lora.lora_request_from_specs' result): the regional LoRA
    scales of THIS request on a pipeline with adapters loaded - set for the call, restored after it; absent / None: the pipeline as it is.
    `param['control']` (optional; set_control's keyword arguments, controlnet.control_from_request / check_control_args' result: image=
    a file, scale=, regions=, negative=, start=, end=): the ControlNet hint and scales of THIS request on a pipeline with a ControlNet
    loaded - set for the call, restored after it; the hint is resized to the request's height x width; absent / None: the pipeline as it is.
    `param['pag']` (optional; set_pag's keyword arguments, pag.pag_from_request / check_pag_args' result: scale=, regions=, base=,
    layers=): perturbed-attention guidance of THIS request in both passes - set for the call, restored after it; absent / None: the
    pipeline as it is."""
    args = (model_type, run_dir, color_guidance_weight, inject_selfattn, segment_threshold, num_segments, inject_background, latents,
            init_image, strength, keep_source)
    pg = param.get('pag')
    if pg is not None:
        keep_pg = getattr(model, 'pag', None)
        model.set_pag(**pg)
        try:
            return generate(model, {k: v for k, v in param.items() if k != 'pag'}, *args)
        finally:
            model.pag = keep_pg
    rl = param.get('region_loras')
    if rl is not None:
        if not getattr(model, 'regional_loras', None):
            raise ValueError("region_loras needs regional LoRA adapters: none is loaded on this pipeline (load_regional_loras / --region_lora)")
        keep_rl = getattr(model, 'lora_request', None)
        model.set_lora_scales(**rl)
        try:
            return generate(model, {k: v for k, v in param.items() if k != 'region_loras'}, *args)
        finally:
            model.lora_request = keep_rl
    cn = param.get('control')
    if cn is not None:
        if getattr(model, 'controlnet', None) is None:
            raise ValueError("control needs a ControlNet: none is loaded on this pipeline (load_controlnet / --controlnet)")
        keep_cn = getattr(model, 'control', None)
        model.set_control(**cn)
        try:
            return generate(model, {k: v for k, v in param.items() if k != 'control'}, *args)
        finally:
            model.control = keep_cn
    ip = param.get('image_prompts')
    if ip is not None:
        from .ip_adapter import apply_specs
        keep_ip = getattr(model, 'image_prompts', None)
        apply_specs(model, ip)
        try:
            return generate(model, {k: v for k, v in param.items() if k != 'image_prompts'}, *args)
        finally:
            model.image_prompts = keep_ip
    fu = param.get('freeu')
    if fu is None:
        return _generate(model, param, *args)
    from .freeu import check_freeu
    fu, keep = check_freeu(fu, "param['freeu']"), getattr(model, 'freeu', None)
    model.enable_freeu(*fu)
    try:
        return _generate(model, param, *args)
    finally:
        model.freeu = keep


def _generate(model, param, model_type, run_dir, color_guidance_weight, inject_selfattn, segment_threshold, num_segments, inject_background,
              latents, init_image, strength, keep_source):
    """The body of generate(): the request as given, on the pipeline as it stands."""
    # the request's own choice, else the one the model was built with; passed to every call below, the model is not changed
    chunks = check_max_prompt_chunks(param.get('max_prompt_chunks') or getattr(model, 'max_prompt_chunks', 1))
    if run_dir:
        os.makedirs(run_dir, exist_ok=True)
    spans = parse_json(param['text_input'], device=model.device)
    base_text_prompt, style_p, note_p, note_tok, color_p, color_names, color_rgbs, sizes, use_grad_guidance = spans
    region_text_prompts, region_target_token_ids, base_tokens = get_region_diffusion_input(
        model, base_text_prompt, style_p, note_p, note_tok, color_p, color_names, max_prompt_chunks=chunks)
    text_format_dict = get_attention_control_input(model, base_tokens, sizes, device=model.device, max_prompt_chunks=chunks)
    text_format_dict, color_target_token_ids = get_gradient_guidance_input(
        model, base_tokens, color_p, color_rgbs, text_format_dict, color_guidance_weight=color_guidance_weight, max_prompt_chunks=chunks)
    height, width, seed, negative_text = param['height'], param['width'], param['noise_index'], param['negative_prompt']
    timings = {}

    seed_everything(seed)
    phi = param.get('guidance_rescale')
    rescale = {} if phi is None else {'guidance_rescale': float(phi)}
    start = {}
    if init_image is not None:
        from . import img2img
        x0 = img2img.source_latents(model, init_image)
        start = dict(image=x0, strength=strength, noise=torch.randn(x0.shape, device=model.device))
    t0 = time.time()
    if model.attention_maps is None:
        model.register_tokenmap_hooks()
    else:
        model.reset_attention_maps()
    if model_type == 'SD':
        plain_img = model.produce_attn_maps([base_text_prompt], [negative_text], height=height, width=width,
                                            num_inference_steps=param['steps'], guidance_scale=param['guidance_weight'], latents=latents, max_prompt_chunks=chunks, noise_seed=seed, **rescale, **start)
    else:
        plain_img = model.sample([base_text_prompt], negative_prompt=[negative_text], height=height, width=width,
                                 num_inference_steps=param['steps'], guidance_scale=param['guidance_weight'], run_rich_text=False,
                                 latents=latents, max_prompt_chunks=chunks, noise_seed=seed, **rescale, **start)
    timings['plain'] = time.time() - t0

    t0 = time.time()
    seed_everything(seed)
    split = bool(getattr(model, 'split_image', False))
    capture_rank, my_rank = 0, 0
    if split:
        # --split_image: the plain pass ran one stream per rank (launcher.split_plain_step), so only the rank of the TEXT stream holds the
        # recorded maps: it derives the masks and hands them to the others (a few hundred KB) - every rank then holds identical masks by
        # construction (the rich pass still digests them, region_diffusion*.py: assert_ranks_agree)
        import torch.distributed as dist
        from .launcher import broadcast_objects, plain_capture_rank
        capture_rank, my_rank = plain_capture_rank(), (dist.get_rank() if dist.is_initialized() else 0)
    if my_rank == capture_rank:
        seg_cache = {}       # both calls cluster the same recorded maps with the same seed: the second reuses the first's segmentation
        color_obj_masks = get_token_maps(model.selfattn_maps, model.crossattn_maps, model.n_maps, run_dir, height // 8, width // 8,
                                         color_target_token_ids[:-1], seed, base_tokens, segment_threshold=segment_threshold,
                                         num_segments=num_segments, cache=seg_cache)
        seed_everything(seed)
        region_masks = get_token_maps(model.selfattn_maps, model.crossattn_maps, model.n_maps, run_dir, height // 8, width // 8,
                                      region_target_token_ids[:-1], seed, base_tokens, segment_threshold=segment_threshold,
                                      num_segments=num_segments, cache=seg_cache)
    else:
        color_obj_masks = region_masks = None
    if split:
        dev = None if color_obj_masks is None else color_obj_masks[-1].device
        packed = None if color_obj_masks is None else ([m.cpu() for m in color_obj_masks], [m.cpu() for m in region_masks])
        color_obj_masks, region_masks = broadcast_objects(packed, capture_rank)
        dev = dev if dev is not None else getattr(model, 'device', 'cpu')
        color_obj_masks, region_masks = [m.to(dev) for m in color_obj_masks], [m.to(dev) for m in region_masks]
    color_obj_atten_all = torch.zeros_like(color_obj_masks[-1])
    for m in color_obj_masks[:-1]:
        color_obj_atten_all += m
    text_format_dict['color_obj_atten'] = [_resize_bicubic_aa(m, height, width) for m in color_obj_masks]
    text_format_dict['color_obj_atten_all'] = color_obj_atten_all
    seed_everything(seed)
    model.masks = region_masks
    model.remove_tokenmap_hooks()
    timings['token_maps'] = time.time() - t0

    t0 = time.time()
    seed_everything(seed)
    if start:
        start['keep_source'] = keep_source
    if model_type == 'SD':
        rich_img = model.prompt_to_img(region_text_prompts, [negative_text], height=height, width=width,
                                       num_inference_steps=param['steps'], guidance_scale=param['guidance_weight'],
                                       use_guidance=use_grad_guidance, inject_selfattn=inject_selfattn,
                                       text_format_dict=text_format_dict, inject_background=inject_background, latents=latents, max_prompt_chunks=chunks, noise_seed=seed, **rescale, **start)
    else:
        rich_img = _xl_rich_pass(model, phi, region_text_prompts, negative_prompt=[negative_text], height=height, width=width,
                                num_inference_steps=param['steps'], guidance_scale=param['guidance_weight'],
                                use_guidance=use_grad_guidance, inject_selfattn=inject_selfattn, text_format_dict=text_format_dict,
                                inject_background=inject_background, run_rich_text=True, latents=latents, max_prompt_chunks=chunks, noise_seed=seed, **start)
    timings['rich'] = time.time() - t0
    return plain_img, rich_img, timings


def _xl_rich_pass(model, phi, *args, **kw):
    """model.sample(run_rich_text=True) with the request's guidance_rescale as the pipeline attribute for the duration of the call (the
    keyword raises there, xl.py:827-830); phi None: the call as it is."""
    if phi is None:
        return model.sample(*args, **kw)
    keep = getattr(model, 'guidance_rescale', 0.0)
    model.guidance_rescale = float(phi)
    try:
        return model.sample(*args, **kw)
    finally:
        model.guidance_rescale = keep


def _load_json_arg(v):
    """`--rich_text_json` value: the JSON text itself (as the reference passes it, sample.py:123) or a path to a file holding it."""
    if os.path.isfile(v):
        with open(v) as f:
            return json.load(f)
    return json.loads(v)


def _request_scheduler(a, name):
    """A --requests line's "scheduler": checked like the flag (an unknown name or one the model cannot run ends the run).  A line without
    the key (None) runs on the flag's scheduler; "default" is not a name a line may use (it would be ambiguous between the flag's
    scheduler and the pipeline's own): leave the key out instead."""
    if name is None:
        return None
    names = [c for c in SCHEDULER_CHOICES if c != 'default']
    if name not in names:
        raise SystemExit(f"sample: --requests: unknown scheduler {name!r} (one of {', '.join(names)}; no key = the --scheduler flag's)")
    order = getattr(a, 'solver_order', None) if name in ('dpmsolver++', 'sde-dpmsolver++') else None
    make_scheduler(types.SimpleNamespace(scheduler=name, solver_order=order, model=getattr(a, 'model', 'SDXL'),
                                         prediction_type=getattr(a, 'prediction_type', None), timestep_spacing=getattr(a, 'timestep_spacing', None)))
    return name


def check_freeu_arg(values, who):
    """--freeu / a --requests line's "freeu": four finite numbers > 0, else the run ends (SystemExit); None stays None."""
    if values is None:
        return None
    from .freeu import check_freeu
    try:
        return list(check_freeu(values, who))
    except ValueError as e:
        raise SystemExit(f"sample: {e}")


def check_requests_freeu(path):
    """The "freeu" keys of a --requests file, checked on their own: main() calls this before any rank starts."""
    with open(path) as f:
        for n, line in enumerate(f, 1):
            if line.strip():
                check_freeu_arg(json.loads(line).get("freeu"), f"--requests line {n}: freeu")


def check_ip_args(a):
    """--ip_adapter / --image_encoder / --ip_image_embeds / --ip_images and the "image_prompts" keys of a --requests file, checked before
    any rank starts: the adapter, the encoder directory and every embedding / image file exist, every FILE[:TARGET[:SCALE]] parses, no
    image prompt without an adapter, no picture without an encoder.  Bad values end the run (SystemExit).  Returns the flags' image
    prompts (ip_adapter.image_prompts_from_specs) or None."""
    from .ip_adapter import image_prompts_from_specs

    def parse(specs, who, images=None, who_images="--ip_images"):
        try:
            ip = image_prompts_from_specs(specs, who, images, who_images)
            entries = [e for e in [ip["base"], ip["negative"], *ip["regions"].values()] if e is not None]
            for e in entries:
                if not os.path.isfile(e.get("file", e.get("image_file"))):
                    raise ValueError(f"{who_images if 'image_file' in e else who}: file not found: {e.get('file', e.get('image_file'))}")
        except ValueError as e:
            raise SystemExit(f"sample: {e}")
        pictures = any("image_file" in e for e in entries)
        if not getattr(a, "ip_adapter", None):
            raise SystemExit(f"sample: {who_images if pictures and not specs else who} needs --ip_adapter")
        if pictures and not getattr(a, "image_encoder", None):
            raise SystemExit(f"sample: {who_images if images else who} needs --image_encoder")
        return ip
    if getattr(a, "ip_adapter", None) and not os.path.isfile(a.ip_adapter):
        raise SystemExit(f"sample: --ip_adapter: file not found: {a.ip_adapter}")
    if getattr(a, "image_encoder", None) and not os.path.isfile(os.path.join(a.image_encoder, "config.json")):
        raise SystemExit(f"sample: --image_encoder: file not found: {os.path.join(a.image_encoder, 'config.json')}")
    embeds, images = getattr(a, "ip_image_embeds", None), getattr(a, "ip_images", None)
    flag = parse(embeds, "--ip_image_embeds", images) if (embeds or images) else None
    if getattr(a, "requests", None):
        with open(a.requests) as f:
            for n, line in enumerate(f, 1):
                if line.strip() and json.loads(line).get("image_prompts") is not None:
                    parse(json.loads(line)["image_prompts"], f"--requests line {n}: image_prompts")
    return flag


def check_control_args(a):
    """--controlnet / --control_image / --control_scale / --control_start / --control_end and the "control" keys of a --requests file,
    checked before any rank starts: the checkpoint and every hint image exist, every scale parses, no control without a ControlNet.  Bad
    values end the run (SystemExit).  Returns the flags' control request (set_control's keyword arguments) or None."""
    from .controlnet import control_from_request, parse_scale_args

    def checked(kw, who):
        if not getattr(a, "controlnet", None):
            raise SystemExit(f"sample: {who} needs --controlnet")
        if not os.path.isfile(kw["image"]):
            raise SystemExit(f"sample: {who}: file not found: {kw['image']}")
        if not (0.0 <= kw["start"] < kw["end"] <= 1.0):
            raise SystemExit(f"sample: {who}: need 0 <= start < end <= 1, got start {kw['start']}, end {kw['end']}")
        return kw
    cn = getattr(a, "controlnet", None)
    if cn and not (os.path.isfile(cn) or os.path.isdir(cn)):
        raise SystemExit(f"sample: --controlnet: file not found: {cn}")
    flag = None
    image = getattr(a, "control_image", None)
    if image:
        try:
            kw = parse_scale_args(getattr(a, "control_scale", None))
        except ValueError as e:
            raise SystemExit(f"sample: {e}")
        kw.update(image=image, start=float(getattr(a, "control_start", 0.0)), end=float(getattr(a, "control_end", 1.0)))
        flag = checked(kw, "--control_image")
    elif getattr(a, "control_scale", None):
        raise SystemExit("sample: --control_scale needs --control_image")
    if getattr(a, "requests", None):
        with open(a.requests) as f:
            for n, line in enumerate(f, 1):
                if line.strip() and json.loads(line).get("control") is not None:
                    try:
                        checked(control_from_request(json.loads(line)["control"], f"--requests line {n}: control"), f"--requests line {n}: control")
                    except ValueError as e:
                        raise SystemExit(f"sample: {e}")
    return flag


def check_pag_args(a):
    """--pag_scale / --pag_layers and the "pag" keys of a --requests file, checked before any rank starts: every scale and layer spec
    parses, and the two refused combinations - no classifier-free guidance (--guidance_weight 0), --guidance_rescale > 0 - end the run
    (SystemExit).  Returns the flags' request (set_pag's keyword arguments) or None."""
    from .pag import DEFAULT_LAYERS, check_guidance, check_layer_forms, pag_from_request, parse_scale_args

    def checked(kw, who):
        try:
            check_layer_forms(kw["layers"])                         # the forms alone: the modules are the UNet's, known once it is loaded
            on = [kw["scale"]] + list(kw["regions"].values()) + ([] if kw["base"] is None else [kw["base"]])
            check_guidance(on, getattr(a, "guidance_weight", 1.0), getattr(a, "guidance_rescale", None) or 0.0, who)
        except ValueError as e:
            raise SystemExit(f"sample: {e}")
        return kw
    flag = None
    if getattr(a, "pag_scale", None):
        try:
            kw = parse_scale_args(a.pag_scale)
        except ValueError as e:
            raise SystemExit(f"sample: {e}")
        kw["layers"] = tuple(getattr(a, "pag_layers", None) or DEFAULT_LAYERS)
        flag = checked(kw, "--pag_scale")
    elif getattr(a, "pag_layers", None):
        raise SystemExit("sample: --pag_layers needs --pag_scale")
    if getattr(a, "requests", None):
        with open(a.requests) as f:
            for n, line in enumerate(f, 1):
                if line.strip() and json.loads(line).get("pag") is not None:
                    try:
                        checked(pag_from_request(json.loads(line)["pag"], f"--requests line {n}: pag"), f"--requests line {n}: pag")
                    except ValueError as e:
                        raise SystemExit(f"sample: {e}")
    return flag


def _request_pag(a, r):
    """A --requests line's "pag" (S | [S, "TARGET:S", ...] | {"scale": ..., "layers": [...]}), else the flags'."""
    if r.get("pag") is None:
        return getattr(a, "pag", None)
    from .pag import pag_from_request
    try:
        return pag_from_request(r["pag"], "--requests: pag")
    except ValueError as e:
        raise SystemExit(f"sample: {e}")


def check_region_lora_args(a):
    """--region_lora and the "region_loras" keys of a --requests file, checked before any rank starts: every file exists, every spec
    parses, at most four adapters in all.  Bad values end the run (SystemExit).  Sets a.region_lora_files = {name: path} of every adapter
    the run loads and returns the flags' request (set_lora_scales' keyword arguments) or None."""
    from .regional_lora import MAX_ADAPTERS, lora_request_from_specs
    files, flag = {}, None

    def parse(specs, who):
        try:
            f, req = lora_request_from_specs(specs, who)
        except ValueError as e:
            raise SystemExit(f"sample: {e}")
        for name, path in f.items():
            if not os.path.isfile(path):
                raise SystemExit(f"sample: {who}: file not found: {path}")
            if files.setdefault(name, path) != path:
                raise SystemExit(f"sample: {who}: two adapter files share the name {name!r}: {files[name]} and {path}")
        return req
    if getattr(a, "region_lora", None):
        flag = parse(a.region_lora, "--region_lora")
    if getattr(a, "requests", None) and os.path.isfile(a.requests):
        with open(a.requests) as f:
            for n, line in enumerate(f, 1):
                if line.strip() and json.loads(line).get("region_loras") is not None:
                    parse(json.loads(line)["region_loras"], f"--requests line {n}: region_loras")
    if len(files) > MAX_ADAPTERS:
        raise SystemExit(f"sample: --region_lora / region_loras name {len(files)} adapters; at most {MAX_ADAPTERS} can be resident")
    a.region_lora_files = files
    return flag


def _request_region_loras(a, r):
    """A --requests line's "region_loras" (["PATH[:TARGET[:SCALE]]", ...], files the run has loaded), else the flags'."""
    if r.get("region_loras") is None:
        return getattr(a, "region_loras", None)
    from .regional_lora import lora_request_from_specs
    try:
        return lora_request_from_specs(r["region_loras"], "--requests: region_loras")[1]
    except ValueError as e:
        raise SystemExit(f"sample: {e}")


def _request_control(a, r):
    """A --requests line's "control" ({"image": FILE, "scale": S | [S, "TARGET:S", ...], "start": a, "end": b}), else the flags'."""
    if r.get("control") is None:
        return getattr(a, "control", None)
    from .controlnet import control_from_request
    try:
        return control_from_request(r["control"], "--requests: control")
    except ValueError as e:
        raise SystemExit(f"sample: {e}")


def _request_image_prompts(a, r):
    """A --requests line's "image_prompts" (a list of FILE[:TARGET[:SCALE]] strings or {"file", "target", "scale"} objects for embeddings,
    or {"embeds": [...], "images": [...]} with the same lists for embeddings and pictures), else the flags'."""
    if r.get("image_prompts") is None:
        return getattr(a, "image_prompts", None)
    from .ip_adapter import image_prompts_from_specs
    try:
        return image_prompts_from_specs(r["image_prompts"], "--requests: image_prompts")
    except ValueError as e:
        raise SystemExit(f"sample: {e}")


def build_requests(a):
    """The (rich-text JSON, seed) list of one invocation.  One JSON + one --seed = the reference's single image.  Several JSONs and / or
    several --seeds = independent requests (BASELINE configs 4 / 5: "batch of 8 independent rich-text JSON/seeds"): JSONs and seeds
    pair up one to one when both lists have the same length, otherwise every JSON is sampled with every seed.  `--requests FILE`:
    one JSON object per line, {"rich_text_json": {...} | "<path>", "seed": 3, "negative_prompt": "...", "scheduler": "euler-ancestral"}
    (missing keys: the flags; "freeu": [s1, s2, b1, b2] = FreeU for that request alone; "image_prompts": ["FILE[:TARGET[:SCALE]]", ...] = the image prompts of that request alone (--ip_adapter); "control": {"image": FILE, "scale": S | [S, "TARGET:S", ...], "start": a, "end": b} = the ControlNet hint and scales of that request alone (--controlnet); "region_loras": ["PATH[:TARGET[:SCALE]]", ...] = the regional LoRA scales of that request alone (every PATH is loaded at start-up, at most four in all); "pag": S | [S, "TARGET:S", ...] | {"scale": ..., "layers": [SPEC, ...]} = perturbed-attention guidance for that request alone; a line's scheduler is one of --scheduler's names other than default and takes --solver_order where that applies)."""
    reqs = []
    if a.requests:
        with open(a.requests) as f:
            for line in f:
                line = line.strip()
                if not line:
                    continue
                r = json.loads(line)
                js = r["rich_text_json"]
                reqs.append(dict(text_input=_load_json_arg(js) if isinstance(js, str) else js, seed=int(r.get("seed", a.seed)),
                                 negative_prompt=r.get("negative_prompt", a.negative_prompt), scheduler=_request_scheduler(a, r.get("scheduler")),
                                 max_prompt_chunks=check_max_prompt_chunks(int(r.get("max_prompt_chunks", getattr(a, "max_prompt_chunks", 1)))),
                                 freeu=check_freeu_arg(r.get("freeu", getattr(a, "freeu", None)), "--requests: freeu"),
                                 image_prompts=_request_image_prompts(a, r), control=_request_control(a, r), region_loras=_request_region_loras(a, r),
                                 pag=_request_pag(a, r)))
    jsons = [_load_json_arg(v) for v in (a.rich_text_json or [])]
    seeds = list(a.seeds) if a.seeds else [a.seed]
    if jsons:
        pairs = list(zip(jsons, seeds)) if len(jsons) == len(seeds) else [(j, sd) for j in jsons for sd in seeds]
        reqs += [dict(text_input=j, seed=int(sd), negative_prompt=a.negative_prompt, max_prompt_chunks=getattr(a, "max_prompt_chunks", 1),
                      freeu=check_freeu_arg(getattr(a, "freeu", None), "--freeu"), image_prompts=getattr(a, "image_prompts", None), control=getattr(a, "control", None), region_loras=getattr(a, "region_loras", None),
                      pag=getattr(a, "pag", None)) for j, sd in pairs]
    if not reqs:
        raise SystemExit("sample: no request (pass --rich_text_json JSON [JSON ...] and / or --requests FILE)")
    for i, r in enumerate(reqs):
        r["index"] = i
    return reqs


def build_model(a, rank=0, local_rank=0, world=1):
    """sample.py:24-32.  world > 1: rank 0 reads the checkpoint, the other ranks build the same objects from the config / tokenizer
    files alone and receive the packed UNet arena, the VAE arena and the text-encoder weights in launcher.broadcast_pipeline's three
    collectives (RCCL over xGMI; SURVEY 8e: one broadcast at start-up, no per-step collectives)."""
    from .region_diffusion import RegionDiffusion
    from .region_diffusion_sdxl import RegionDiffusionXL
    res = 512 if a.model == 'SD' else 1024
    # the VAE plan (decode + colour guidance workspace) is sized for the requested image, like the UNet engine
    hw = ((a.height or res) // 8, (a.width or res) // 8)
    def with_adapter(m):          # --ip_adapter: every rank reads the file itself (the small image_proj tensors; the layer weights travel in the arena)
        if getattr(a, 'ip_adapter', None):
            try:
                m.load_ip_adapter(a.ip_adapter)
            except ValueError as e:
                raise SystemExit(f"sample: --ip_adapter: {e}")
        if getattr(a, 'image_encoder', None):    # --image_encoder: read and checked on every rank, on the GPU with the first picture
            try:
                m.load_image_encoder(a.image_encoder)
            except ValueError as e:
                raise SystemExit(f"sample: --image_encoder: {e}")
        if getattr(a, 'controlnet', None):       # --controlnet: every rank reads the file itself and checks it; on ranks > 0 the weights travel in the arena
            try:
                m.load_controlnet(a.controlnet)
            except ValueError as e:
                raise SystemExit(f"sample: --controlnet: {e}")
        if getattr(a, 'region_lora_files', None):    # --region_lora: every rank reads the files itself (the column map is per engine; the factors travel in the arena)
            try:
                m.load_regional_loras(a.region_lora_files, attention_only=bool(getattr(a, 'region_lora_attention_only', False)),
                                      targets=getattr(a, 'region_lora_targets', None) or 'attention')
            except (ValueError, KeyError) as e:
                raise SystemExit(f"sample: --region_lora: {e}")
        return m
    if world == 1:
        if a.model == 'SD':
            return apply_scheduler(with_adapter(RegionDiffusion(torch.device('cuda'), load_path=a.load_path, latent_hw=hw)), a), 0.0
        xl_path = a.load_path or ("stabilityai/stable-diffusion-xl-base-1.0" if a.model == 'SDXL' else "Linaqruf/animagine-xl")
        model = RegionDiffusionXL(load_path=xl_path, latent_hw=hw)
        if getattr(a, 'guidance_precision', 'fp32') == 'bf16':
            from .checkpoint import load_guidance_vae, resolve_checkpoint
            model.guidance_vae = load_guidance_vae(resolve_checkpoint(xl_path, 'SDXL'), 'SDXL', 0, hw)
        return apply_scheduler(with_adapter(model), a), 0.0
    from . import launcher
    from .checkpoint import load_components, resolve_checkpoint
    kind = 'SD' if a.model == 'SD' else 'SDXL'
    default = None if a.model != 'AnimeXL' else "Linaqruf/animagine-xl"
    comp = load_components(resolve_checkpoint(a.load_path or default, kind), kind, local_rank, hw, weights=(rank == 0))
    if kind == 'SD':
        model = RegionDiffusion(local_rank, **comp)
        encoders = [comp["text_encoder"].enc]
    else:
        model = RegionDiffusionXL(None, local_rank, **comp)
        encoders = list(comp["text_encoders"].encoders)
    with_adapter(model)                                              # before the engine exists: its arena holds the adapter's projections
    eng = model.unet.engine(hw[0], hw[1])                            # the engine (and its arena) must exist on every rank before the broadcast
    seconds = launcher.broadcast_pipeline(eng, model.vae, encoders, src=0, pipeline=model)
    return apply_scheduler(model, a), seconds


def load_init_image(path, height, width):
    """--init_image: the file as RGB, resized to height x width -> [1,3,height,width] in [0,1]."""
    import numpy as np
    from PIL import Image
    img = Image.open(path).convert('RGB').resize((width, height), Image.BICUBIC)
    return torch.from_numpy(np.asarray(img, dtype=np.float32) / 255.0).permute(2, 0, 1)[None].contiguous()


SCHEDULER_CHOICES = ['default', 'dpmsolver++', 'sde-dpmsolver++', 'euler-ancestral']


def make_scheduler(a):
    """--scheduler / --solver_order -> the scheduler object to put on the pipeline (None: the pipeline's default, PNDM for SD and
    Euler for SDXL).  A flag that cannot be honoured is an error, never ignored."""
    from .schedulers import DPMSolverTables, EulerAncestralTables, EulerTables, PNDMTables
    order = getattr(a, 'solver_order', None)
    name = getattr(a, 'scheduler', 'default')
    # --prediction_type / --timestep_spacing: keywords of whichever tables run (None: the tables' / the checkpoint's default)
    kw = {k: getattr(a, k) for k in ('prediction_type', 'timestep_spacing') if getattr(a, k, None) is not None}
    phi = getattr(a, 'guidance_rescale', None)
    if phi is not None and not (0.0 <= phi <= 1.0):
        raise SystemExit(f"sample: --guidance_rescale must be in [0, 1], got {phi}")
    try:
        if name in ('dpmsolver++', 'sde-dpmsolver++'):
            return DPMSolverTables(solver_order=2 if order is None else order, algorithm=name, **kw)
        if order is not None:
            raise SystemExit("sample: --solver_order needs --scheduler dpmsolver++ or sde-dpmsolver++")
        if name == 'euler-ancestral':
            if getattr(a, 'model', 'SD') == 'SD':
                raise SystemExit("sample: --scheduler euler-ancestral runs in sigma space: --model SDXL or AnimeXL only "
                                 "(--model SD: sde-dpmsolver++ is its stochastic sampler)")
            return EulerAncestralTables(**kw)
        if kw:                            # the pipeline's default sampler with the flags' keywords (PNDM refuses trailing spacing)
            return (PNDMTables if getattr(a, 'model', 'SD') == 'SD' else EulerTables)(**kw)
    except ValueError as e:
        raise SystemExit(f"sample: {e}")
    return None


def apply_scheduler(model, a):
    sched = make_scheduler(a)
    if sched is not None:
        if getattr(a, 'prediction_type', None) is None:        # no flag: what the checkpoint's scheduler_config.json said stays
            sched.prediction_type = getattr(getattr(model, 'scheduler', None), 'prediction_type', 'epsilon')
        model.scheduler = sched
    return model


def apply_request_scheduler(model, flag_scheduler, r, a):
    """The scheduler request `r` runs on: the one its --requests line names (with --solver_order where that applies), else
    `flag_scheduler`, what --scheduler left on the pipeline.  Set for every request, so a line's choice never leaks into the next."""
    model.scheduler = flag_scheduler
    name = r.get('scheduler')
    if name is not None:
        apply_scheduler(model, types.SimpleNamespace(scheduler=name, model=a.model,
                                                     solver_order=a.solver_order if name in ('dpmsolver++', 'sde-dpmsolver++') else None,
                                                     prediction_type=getattr(a, 'prediction_type', None),
                                                     timestep_spacing=getattr(a, 'timestep_spacing', None)))
    return model


def dist_backend_is_gloo():
    import torch.distributed as dist
    return dist.is_initialized() and dist.get_backend() == "gloo"


def build_parser():
    """The flags of main()."""
    p = argparse.ArgumentParser()
    p.add_argument('--run_dir', type=str, default='results/')
    p.add_argument('--height', type=int, default=None)
    p.add_argument('--width', type=int, default=None)
    p.add_argument('--seed', type=int, default=6)
    p.add_argument('--sample_steps', type=int, default=41)
    p.add_argument('--rich_text_json', type=str, nargs='+', default=None, help='JSON text or a file holding it; several = independent requests')
    p.add_argument('--negative_prompt', type=str, default='')
    p.add_argument('--max_prompt_chunks', type=int, default=1, choices=(1, 2, 3),
                   help='75-token CLIP windows a text may span (chunked and concatenated: 77 cross-attention keys per window); 1 = cut at 77 tokens, '
                        'as the reference does.  A text that needs more windows than allowed is an error, never cut silently')
    p.add_argument('--model', type=str, default='SD', choices=['SD', 'SDXL', 'AnimeXL'])
    p.add_argument('--guidance_weight', type=float, default=8.5)
    p.add_argument('--color_guidance_weight', type=float, default=0.5)
    p.add_argument('--inject_selfattn', type=float, default=0.)
    p.add_argument('--segment_threshold', type=float, default=0.3)
    p.add_argument('--num_segments', type=int, default=9)
    p.add_argument('--inject_background', type=float, default=0.)
    p.add_argument('--guidance_precision', type=str, default='fp32', choices=['fp32', 'bf16'],
                   help='SDXL colour guidance: fp32 = the fp32-class VAE the reference guides with (xl.py:856; default), bf16 = the guidance pass '
                        'alone on a one-pass bf16 VAE engine (same trajectory within the bf16 noise of the UNet, 37 instead of 80 ms per step); '
                        'the final decode stays fp32-class either way')
    p.add_argument('--scheduler', type=str, default='default', choices=SCHEDULER_CHOICES,
                   help='default: the reference\'s sampler (PNDM for SD, Euler for SDXL / AnimeXL); dpmsolver++: DPM-Solver++ multistep '
                        '(diffusers DPMSolverMultistepScheduler), usually run at 20-25 --sample_steps; sde-dpmsolver++ ("DPM++ 2M SDE") and '
                        'euler-ancestral ("Euler a", SDXL / AnimeXL only): their stochastic forms, fresh noise at every step, made on the GPU '
                        'from the request\'s seed. Holds on every rank of --gpus N')
    p.add_argument('--solver_order', type=int, default=None, choices=[1, 2],
                   help='DPM-Solver++ order (default 2); needs --scheduler dpmsolver++ or sde-dpmsolver++')
    p.add_argument('--guidance_rescale', type=float, default=None,
                   help='CFG rescale in [0, 1] (Lin et al., "Common Diffusion Noise Schedules and Sample Steps are Flawed", 3.4): the guided '
                        'prediction is scaled towards the standard deviation of its conditional half, in both passes; made for '
                        'v-prediction checkpoints, usually 0.7.  Default: off')
    p.add_argument('--freeu', type=float, nargs=4, default=None, metavar=('S1', 'S2', 'B1', 'B2'),
                   help='FreeU (diffusers enable_freeu, same order): in the first two up blocks of the UNet the four lowest frequency bins of '
                        'the skip features are scaled by S1 / S2 and half of the backbone channels by B1 / B2, in both passes; all > 0. '
                        'Usual values: SD-v1.5 0.9 0.2 1.5 1.6, SDXL 0.6 0.4 1.1 1.2.  Default: off.  Holds on every rank of --gpus N')
    p.add_argument('--ip_adapter', type=str, default=None, metavar='PATH',
                   help='IP-Adapter checkpoint (.safetensors / .bin, the original layout or diffusers\' names; linear image projection): image '
                        'prompts by decoupled cross-attention, see --ip_image_embeds.  Holds on every rank of --gpus N')
    p.add_argument('--ip_image_embeds', type=str, nargs='+', default=None, metavar='FILE[:TARGET[:SCALE]]',
                   help='with --ip_adapter: a CLIP image embedding (.pt / .npy / .safetensors; a [t, D] matrix = ready image tokens) as the image '
                        'prompt of TARGET = base (default: the whole picture, both passes), negative, or a region number of the rich text '
                        '(that region alone); SCALE defaults to 1')
    p.add_argument('--image_encoder', type=str, default=None, metavar='DIR',
                   help='CLIP vision encoder directory in the Hugging Face layout (config.json + model.safetensors / pytorch_model.bin, '
                        'optionally preprocessor_config.json: IP-Adapter\'s models/image_encoder): turns the pictures of --ip_images into '
                        'image embeddings on the GPU.  At most 640 tokens per image.  Every rank of --gpus N loads its own')
    p.add_argument('--ip_images', type=str, nargs='+', default=None, metavar='FILE[:TARGET[:SCALE]]',
                   help='with --ip_adapter and --image_encoder: a picture (.png / .jpg / .jpeg / .webp / .bmp) as the image prompt of TARGET, '
                        'as --ip_image_embeds; both flags may be given, two prompts for one TARGET are an error')
    p.add_argument('--controlnet', type=str, default=None, metavar='PATH',
                   help='ControlNet checkpoint (.safetensors / .bin in diffusers\' ControlNetModel layout, or its directory) for this UNet: a '
                        'hint image steers the geometry of both passes, see --control_image.  Holds on every rank of --gpus N')
    p.add_argument('--control_image', type=str, default=None, metavar='FILE',
                   help='with --controlnet: the hint (edges, depth, pose, a scribble - already preprocessed), resized to height x width')
    p.add_argument('--control_scale', type=str, nargs='+', default=None, metavar='S|TARGET:S',
                   help='with --control_image: the conditioning scale.  A bare S is the default of every prompt (the negative one included, as '
                        'in diffusers); TARGET:S overrides it for TARGET = negative or a region number of the rich text; base:S is the bare S. '
                        'A prompt with scale 0 is not controlled.  Default 1')
    p.add_argument('--region_lora', type=str, nargs='+', default=None, metavar='PATH[:TARGET[:SCALE]]',
                   help='regional LoRA: adapters (kohya / diffusers / peft layouts, on the attention projections) kept unmerged and scaled per '
                        'prompt.  TARGET: all (default), base, negative or a region number; SCALE default 1.  Up to four files, 128 rank columns '
                        'in all; the same file may be named with several targets.  (load_components(lora_path=) merges ONE adapter into the weights instead)')
    p.add_argument('--region_lora_attention_only', action='store_true',
                   help='with --region_lora: drop a checkpoint\'s tensors on other modules (feed-forward, proj_in / proj_out, resnets) instead of refusing it')
    p.add_argument('--region_lora_targets', choices=('attention', 'transformer'), default='attention',
                   help='with --region_lora: the modules an adapter may sit on - attention: the eight attention projections (default); '
                        'transformer: also ff.net.0.proj, ff.net.2, proj_in and proj_out, kohya\'s default network.  Adapters are loaded once '
                        'per run, so a --requests run uses this value for every line')
    p.add_argument('--pag_scale', type=str, nargs='+', default=None, metavar='S|TARGET:S',
                   help='perturbed-attention guidance in both passes: a bare S is the scale of the base prompt and of every rich-text region, '
                        'TARGET is base or a region number.  A prompt with scale 0 gets no perturbed stream.  Needs classifier-free guidance; '
                        'not together with --guidance_rescale')
    p.add_argument('--pag_layers', type=str, nargs='+', default=None, metavar='SPEC',
                   help='with --pag_scale: the self-attention modules that are perturbed - mid (default), down, up, down_blocks.N, up_blocks.N, '
                        '...attentions.M or full attn1 module names')
    p.add_argument('--control_start', type=float, default=0.0, help='with --control_image: the fraction of the executed schedule at which control begins (control_guidance_start)')
    p.add_argument('--control_end', type=float, default=1.0, help='... and at which it ends (control_guidance_end)')
    p.add_argument('--prediction_type', type=str, default=None, choices=['epsilon', 'v_prediction'],
                   help='what the UNet predicts; default: the checkpoint\'s scheduler/scheduler_config.json, else epsilon')
    p.add_argument('--timestep_spacing', type=str, default=None, choices=['leading', 'trailing'],
                   help='trailing: the schedule starts at the last training timestep (Euler, Euler ancestral and the DPM-Solver++ kinds; '
                        'the SD default sampler PNDM refuses it).  Default: each sampler\'s own list')
    p.add_argument('--init_image', type=str, default=None,
                   help='edit this image instead of starting from noise: it is resized to height x width, encoded once, and both passes '
                        'start from it at --strength')
    p.add_argument('--strength', type=float, default=0.8,
                   help='with --init_image: the share of the schedule that is executed, in (0, 1]; 1 keeps nothing of the image but its '
                        'pinned pixels.  The token maps need more than 10 executed steps')
    p.add_argument('--keep_source', type=str, default='none', choices=['none', 'background'],
                   help='with --init_image: background = the region of the unformatted text stays the image itself (its latents are reset to '
                        'the image at every step of the rich pass)')
    p.add_argument('--load_path', type=str, default=None,
                   help='diffusers-layout checkpoint directory; default: the hub ids of sample.py:26-30 resolved locally '
                        '(checkpoint.resolve_checkpoint: $RTDIFF_SD_PATH / $RTDIFF_SDXL_PATH / the Hugging Face hub cache)')
    p.add_argument('--seeds', type=int, nargs='*', default=None, help='seeds of the independent requests (default: --seed)')
    p.add_argument('--requests', type=str, default=None, help='JSON-lines request file (see build_requests)')
    p.add_argument('--gpus', type=int, default=1, help='ranks = GPUs of this node; requests are dealt round-robin (one engine per GPU)')
    p.add_argument('--split_image', action='store_true',
                   help='with --gpus N: the ranks work on the SAME request - every rich-text step is split by streams (text_ref and the '
                        'region forwards that inject from it on one GPU, the independent forwards on the others), one exchange of the noise '
                        'predictions per step (launcher.split_region_step): lower latency per image instead of more images; bit-identical '
                        'with the one-GPU result.  Rank 0 writes the images.')
    p.add_argument('--dry_launch', action='store_true',
                   help='exercise the launch / sharding / broadcast control path on the gloo backend with stand-in arenas and print '
                        'one JSON line per rank - no GPU, no checkpoint (tests/test_distributed_cpu.py)')
    return p


def main(argv=None):
    """Flags of sample.py:118-133 (+ --load_path), and the seed-parallel form the reference does not have (BASELINE
    configs 4 / 5): `--gpus N` with several requests (`--rich_text_json A B ...`, `--seeds ...`, `--requests FILE`) re-executes itself
    as N ranks under torch.distributed.run, rank 0 loads the checkpoint, ONE pipeline broadcast, requests dealt round-robin, every
    rank writes its own images.  With one GPU and one request this is the reference's main()."""
    import sys
    p = build_parser()
    argv = list(sys.argv[1:] if argv is None else argv)
    a = p.parse_args(argv)
    make_scheduler(a)                 # an unusable --scheduler / --solver_order combination fails here, before any rank starts
    a.freeu = check_freeu_arg(a.freeu, "--freeu")      # ... and so do bad FreeU values, the flag's and a --requests line's
    if a.requests:
        check_requests_freeu(a.requests)
    a.image_prompts = check_ip_args(a)                 # ... and a missing adapter / embedding file or a malformed FILE[:TARGET[:SCALE]]
    a.control = check_control_args(a)                  # ... and a missing ControlNet / hint image or a malformed --control_scale
    a.region_loras = check_region_lora_args(a)         # ... and a missing adapter file or a malformed PATH[:TARGET[:SCALE]]
    a.pag = check_pag_args(a)                          # ... and a malformed --pag_scale / --pag_layers or one of PAG's two refused combinations
    if a.init_image is None and a.keep_source != 'none':
        raise SystemExit("sample: --keep_source needs --init_image")
    if a.init_image is not None and a.keep_source != 'none' and a.split_image:
        raise SystemExit("sample: --keep_source is not supported with --split_image")
    from . import launcher
    err = launcher.self_launch(None, argv, a.gpus, require_gpus=not a.dry_launch, module=__spec__.name if __spec__ else "rich_text_to_image_amd.sample")
    if err is not None:
        raise SystemExit(f"sample: {err}")
    # RTDIFF_DIST_BACKEND / RTDIFF_FORCE_DEVICE: tests that run two ranks on ONE GPU over gloo (RCCL cannot put two ranks on a device)
    rank, local_rank, world = launcher.init_distributed("gloo" if a.dry_launch else os.environ.get("RTDIFF_DIST_BACKEND"))
    if world > 1:                     # prove the collective path before the pipeline's weights move (launcher.collective_self_check)
        chk = launcher.collective_self_check(nbytes=(1 << 20) if a.dry_launch else (64 << 20),
                                             device=torch.device("cpu") if (a.dry_launch or dist_backend_is_gloo()) else None)
        if rank == 0:
            print(f"sample: collective self-check {chk}", file=sys.stderr, flush=True)
    if "RTDIFF_FORCE_DEVICE" in os.environ:
        local_rank = int(os.environ["RTDIFF_FORCE_DEVICE"])
    if world != max(1, a.gpus) and "WORLD_SIZE" in os.environ:
        raise SystemExit(f"sample: --gpus {a.gpus} but the launch environment says WORLD_SIZE={world}")
    reqs = build_requests(a)
    mine = reqs if a.split_image else launcher.shard_round_robin(reqs, rank, world)      # --split_image: every rank runs every request
    if a.dry_launch:
        return _dry_launch(a, rank, world, reqs, mine)
    torch.cuda.set_device(local_rank)
    model, bcast_s = build_model(a, rank, local_rank, world)
    res = 512 if a.model == 'SD' else 1024
    model.split_image = bool(a.split_image and world > 1)
    os.makedirs(a.run_dir, exist_ok=True)
    from PIL import Image
    init_image = load_init_image(a.init_image, a.height or res, a.width or res) if a.init_image else None
    out = []
    flag_scheduler = model.scheduler
    for r in mine:
        apply_request_scheduler(model, flag_scheduler, r, a)
        param = {'text_input': r['text_input'], 'height': a.height or res, 'width': a.width or res, 'guidance_weight': a.guidance_weight,
                 'steps': a.sample_steps, 'noise_index': r['seed'], 'negative_prompt': r['negative_prompt'],
                 'max_prompt_chunks': r.get('max_prompt_chunks', 1), 'guidance_rescale': a.guidance_rescale, 'freeu': r.get('freeu'), 'image_prompts': r.get('image_prompts'),
                 'control': r.get('control'), 'region_loras': r.get('region_loras'), 'pag': r.get('pag')}
        plain, rich, t = generate(model, param, 'SD' if a.model == 'SD' else 'SDXL', a.run_dir, a.color_guidance_weight, a.inject_selfattn,
                                  a.segment_threshold, a.num_segments, a.inject_background, init_image=init_image, strength=a.strength,
                                  keep_source=None if a.keep_source == 'none' else a.keep_source)
        print('[rank %d] request %d seed %d: time lapses: plain %.3f s, token maps %.3f s, rich %.3f s'
              % (rank, r['index'], r['seed'], t['plain'], t['token_maps'], t['rich']), flush=True)
        # seed%d_plain.jpg / seed%d_rich.jpg in run_dir, as sample.py:62-76,97-112 writes them (imageio there, PIL here); with several
        # requests the request index keeps the names apart
        tag = 'seed%d' % r['seed'] if len(reqs) == 1 else 'req%d_seed%d' % (r['index'], r['seed'])
        for name, img in (('plain', plain), ('rich', rich)):
            if a.split_image and rank != 0:           # every rank holds the same image: rank 0 writes it
                continue
            arr = img.images[0] if hasattr(img, 'images') else img[0]
            (arr if isinstance(arr, Image.Image) else Image.fromarray(arr)).save(os.path.join(a.run_dir, '%s_%s.jpg' % (tag, name)))
        out.append((plain, rich))
    launcher.barrier()
    if world > 1:
        if rank == 0:
            print('sample: %d requests on %d ranks, pipeline broadcast %.3f s (%d collectives)' % (len(reqs), world, bcast_s, launcher.LAST_BROADCAST_CALLS), flush=True)
        torch.distributed.destroy_process_group()
    return out[0] if len(out) == 1 else out


class _StandInArena:
    """CPU stand-in for an Engine / VaeDecoder in the dry launch: a byte arena, `arena_mark_bound`, `synchronize`."""

    def __init__(self, nbytes, fill):
        self.t = torch.full((nbytes,), fill, dtype=torch.uint8) if fill is not None else torch.zeros(nbytes, dtype=torch.uint8)
        self.bound = fill is not None
        self.device = "cpu"

    def arena_as_tensor(self):
        return self.t

    def arena_mark_bound(self):
        self.bound = True

    def synchronize(self):
        pass


class _StandInEncoder:
    def __init__(self, filled):
        g = torch.Generator().manual_seed(7)
        shapes = [((64, 32), torch.float32), ((32,), torch.float32), ((48, 32), torch.bfloat16), ((5,), torch.float32)]
        self.p = [(torch.randn(*s, generator=g).to(dt) if filled else torch.zeros(*s, dtype=dt)) for s, dt in shapes]

    def parameter_tensors(self):
        return self.p


def _dry_launch(a, rank, world, reqs, mine):
    """The control path of a `--gpus N` run without GPUs or checkpoints: the SAME launcher.broadcast_pipeline call build_model makes,
    on stand-in arenas (rank 0 filled, the others zero), then the per-rank request list as one JSON line."""
    from . import launcher
    unet, vae = _StandInArena(1 << 16, 0xA5 if rank == 0 else None), _StandInArena(1 << 12, 0x3C if rank == 0 else None)
    encs = [_StandInEncoder(rank == 0), _StandInEncoder(rank == 0)]
    from .freeu import FreeUMixin
    pipe = FreeUMixin()                              # rank 0 alone holds the flag's values: the others receive them with the pipeline
    if rank == 0 and a.freeu is not None:
        pipe.enable_freeu(*a.freeu)
    seconds = launcher.broadcast_pipeline(unet, vae, encs, src=0, pipeline=pipe)
    ref = _StandInEncoder(True)
    sched = apply_scheduler(types.SimpleNamespace(scheduler=None), a).scheduler        # what build_model puts on this rank's pipeline
    ok = bool((unet.t == 0xA5).all() and (vae.t == 0x3C).all() and unet.bound and vae.bound and
              all(torch.equal(x, y) for e in encs for x, y in zip(e.p, ref.p)))
    # ONE write per rank (line + newline together): the ranks share the launcher's stdout pipe, and print()'s separate newline write let two
    # ranks' lines run into each other once in ~25 runs
    sys.stdout.write(json.dumps({"rank": rank, "world": world, "requests_total": len(reqs), "requests_mine": [r["index"] for r in mine],
                                 "seeds_mine": [r["seed"] for r in mine], "pipeline_received": ok, "broadcast_collectives": launcher.LAST_BROADCAST_CALLS,
                                 "broadcast_s": seconds, "freeu": None if pipe.freeu is None else list(pipe.freeu),
                                 "scheduler": None if sched is None else {"class": type(sched).__name__, "kind": sched.kind,
                                                                          "solver_order": getattr(sched, "solver_order", None)}}) + "\n")
    sys.stdout.flush()
    launcher.barrier()
    if world > 1:
        torch.distributed.destroy_process_group()
    if not ok:
        raise SystemExit("sample: dry launch: pipeline broadcast payload mismatch")
    return None


if __name__ == '__main__':
    main()
