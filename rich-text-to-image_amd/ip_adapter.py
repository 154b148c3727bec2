"""Image prompts (IP-Adapter, Ye et al. 2023: "IP-Adapter: Text Compatible Image Prompt Adapter for Text-to-Image Diffusion Models"): every
attn2 of the UNet gets a second pair of key / value projections over a few image tokens and computes
attn(Q, K_text, V_text) + scale * attn(Q, K_ip, V_ip).  The layer arithmetic runs inside the engine (csrc/ipattn.hip, include/rtdiff.h:
rt_set_image_prompts); this module holds the host side: the checkpoint loader, the image projection (through the engine's small kernels,
once per image) and the pipeline attribute both facades share.  A stream uses the image of the prompt it runs, so a rich-text request
can give every region its own reference image, one to the base prompt, or none.

An entry may also be a picture (`image=`): `load_image_encoder` puts a CLIP vision encoder (clip_vision_encoder.py) on the pipeline, which
encodes the picture once, outside the step.  Without one, image embeddings come from the caller, as prompt_embeds do for SD-2.x.

A "plus" checkpoint carries a Resampler in place of the linear projection (resampler.py): its input is the encoder's penultimate hidden
states, not the pooled embedding, so an entry is then a picture (`image=`), hidden states from the caller (`hidden=[N, E]`) or ready
tokens; `embeds=` is refused.

Not here: FaceID, several adapters at once, per-layer scales, diffusers' renamed IPAdapterPlusImageProjection keys."""
import ctypes as C
import math
import os

MAX_TOKENS = 16          # rt_config.ip_tokens


def attn2_names(config):
    """The attn2 modules of a UNet config in the order of the UNet's attn_processors: down blocks, up blocks, then the mid block - the
    order the original checkpoints number their layers in (ip_adapter.{2 k + 1} = the k-th attn2; the attn1 processors hold no weights)."""
    n = len(config["block_out_channels"])

    def tup(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n
    lpb, tl = tup(config["layers_per_block"]), tup(config["transformer_layers_per_block"])
    boc = tuple(config["block_out_channels"])
    out = []
    for i, bt in enumerate(config["down_block_types"]):
        if bt == "CrossAttnDownBlock2D":
            out += [(f"down_blocks.{i}.attentions.{j}.transformer_blocks.{k}.attn2", boc[i]) for j in range(lpb[i]) for k in range(tl[i])]
    for i, bt in enumerate(config["up_block_types"]):
        if bt == "CrossAttnUpBlock2D":
            out += [(f"up_blocks.{i}.attentions.{j}.transformer_blocks.{k}.attn2", boc[n - 1 - i]) for j in range(lpb[n - 1 - i] + 1)
                    for k in range(tl[n - 1 - i])]
    out += [(f"mid_block.attentions.0.transformer_blocks.{k}.attn2", boc[n - 1]) for k in range(tl[n - 1])]
    return out


def _read_file(path):
    if not os.path.isfile(path):
        raise ValueError(f"IP-Adapter checkpoint not found: {path}")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path)
    import torch
    return torch.load(path, map_location="cpu", weights_only=True)


def _flatten(sd):
    """The nested {"image_proj": {...}, "ip_adapter": {...}} layout -> flat keys."""
    flat = {}
    for k, v in sd.items():
        if isinstance(v, dict):
            flat.update({f"{k}.{kk}": vv for kk, vv in v.items()})
        else:
            flat[k] = v
    return flat


def load_ip_adapter(path_or_state_dict, config, dim_head=64):
    """An IP-Adapter checkpoint for the UNet `config` -> dict(weights = {"<attn2>.to_k_ip.weight" / ".to_v_ip.weight": tensor} under the
    engine's names, image_proj = {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}, T = image tokens per image, D, E).
    Reads the original layout - a .safetensors / .bin file or a dict with flat keys image_proj.* / ip_adapter.{2 k + 1}.to_k_ip.weight, or
    the nested dict - and diffusers' names (<attn2>.processor.to_k_ip.0.weight).  A "plus" checkpoint (image_proj.latents / proj_in /
    layers.* / proj_out / norm_out: a Resampler, resampler.py) gives the same dict with an empty image_proj, E = the Resampler's
    embedding_dim and resampler = resampler.check_resampler's result (`dim_head`: the one dimension its shapes do not tell).  ValueError
    naming the key for a missing or left-over key, a shape that does not match the UNet, or Resampler keys next to proj.*."""
    sd = _read_file(path_or_state_dict) if isinstance(path_or_state_dict, (str, os.PathLike)) else path_or_state_dict
    sd = _flatten(dict(sd))
    D = int(config["cross_attention_dim"])
    proj, rest = {}, {}
    for k, v in sd.items():
        if k.startswith("image_proj."):
            proj[k[len("image_proj."):]] = v
        else:
            rest[k] = v
    linear_keys = ("proj.weight", "proj.bias", "norm.weight", "norm.bias")
    plus_keys = [k for k in proj if k.split(".")[0] in ("latents", "proj_in", "proj_out", "layers", "norm_out")]
    resampler = None
    if plus_keys and not any(k in proj for k in linear_keys):
        from .resampler import check_resampler
        resampler = check_resampler(proj, dim_head)
        if resampler["D"] != D:
            raise ValueError(f"IP-Adapter: image_proj.proj_out.weight has {resampler['D']} rows, the UNet's cross_attention_dim is {D}")
        T, E = resampler["T"], resampler["E"]
        proj = {}
    else:
        for k in proj:
            if k not in linear_keys:
                kind = ("a Resampler (\"plus\") key next to the linear projection's image_proj.proj.* / norm.*: a checkpoint holds one projection"
                        if k in plus_keys else "unknown key")
                raise ValueError(f"IP-Adapter: image_proj.{k}: {kind}")
        for k in linear_keys:
            if k not in proj:
                raise ValueError(f"IP-Adapter: missing key image_proj.{k}")
        rows, E = (int(s) for s in proj["proj.weight"].shape)
        if rows % D != 0 or not 1 <= rows // D <= MAX_TOKENS:
            raise ValueError(f"IP-Adapter: image_proj.proj.weight has {rows} rows: expected T * {D} (cross_attention_dim) with T in 1 .. {MAX_TOKENS}")
        T = rows // D
        for k, shape in (("proj.bias", (rows,)), ("norm.weight", (D,)), ("norm.bias", (D,))):
            if tuple(proj[k].shape) != shape:
                raise ValueError(f"IP-Adapter: image_proj.{k} has shape {tuple(proj[k].shape)}, expected {shape}")
    weights = {}
    for k, (name, Cq) in enumerate(attn2_names(config)):
        for w in ("to_k_ip", "to_v_ip"):
            keys = (f"ip_adapter.{2 * k + 1}.{w}.weight", f"{name}.processor.{w}.0.weight", f"{name}.{w}.weight")
            key = next((c for c in keys if c in rest), None)
            if key is None:
                raise ValueError(f"IP-Adapter: missing key {keys[0]} ({name}.{w})")
            t = rest.pop(key)
            if tuple(t.shape) != (Cq, D):
                raise ValueError(f"IP-Adapter: {key} has shape {tuple(t.shape)}, the UNet's {name} needs {(Cq, D)}")
            weights[f"{name}.{w}.weight"] = t
    if rest:
        raise ValueError(f"IP-Adapter: left-over key {sorted(rest)[0]} ({len(rest)} in all): the checkpoint does not belong to this UNet")
    out = dict(weights=weights, image_proj={k: v.detach().float() for k, v in proj.items()}, T=T, D=D, E=E)
    if resampler is not None:
        out["resampler"] = resampler
    return out


def resample(adapter, hidden, device=0):
    """The Resampler of a plus adapter on ONE image's hidden states [N, E] -> tokens [T, D] fp32 on the GPU (resampler.HipResampler; its
    weights go to the device with the first call).  Once per image, outside the step."""
    import torch
    from .resampler import LazyResampler
    lazy = adapter.get("_resampler")
    if lazy is None:
        lazy = adapter["_resampler"] = LazyResampler(adapter["resampler"])
    return lazy.on(device)(torch.as_tensor(hidden).detach().float()[None])[0]


def project(adapter, image_embeds, device=0):
    """ImageProjection: LayerNorm(Linear(e).reshape(T, D)) of ONE image embedding [E] -> tokens [T, D] fp32 on the GPU, through the engine's
    small-linear and LayerNorm kernels (rt_op_small_linear, rt_op_layernorm; bf16 weights and result, fp32 arithmetic).  Once per image,
    outside the step."""
    import torch
    from .engine import RtError, _ptr, load_library
    lib = load_library()
    dev = f"cuda:{device}"
    T, D, E = adapter["T"], adapter["D"], adapter["E"]
    e = torch.as_tensor(image_embeds).detach().float().reshape(-1)
    if e.numel() != E:
        raise ValueError(f"image embedding of {e.numel()} values: the adapter's projection takes {E}")
    cache = adapter.setdefault("_device", {})
    if device not in cache:
        p = adapter["image_proj"]
        cache[device] = (p["proj.weight"].to(dev).to(torch.bfloat16).contiguous(), p["proj.bias"].to(dev).contiguous(),
                         p["norm.weight"].to(dev).contiguous(), p["norm.bias"].to(dev).contiguous())
    W, b, g, beta = cache[device]
    with torch.cuda.device(dev):
        x = e.to(dev).reshape(1, E).contiguous()
        y = torch.empty(1, T * D, device=dev)
        out = torch.empty(T, D, dtype=torch.bfloat16, device=dev)
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        for call in (lambda: lib.rt_op_small_linear(_ptr(x), E, _ptr(W), E, _ptr(b), _ptr(y), T * D, 1, T * D, E, 0, 0, st),
                     lambda: lib.rt_op_layernorm(_ptr(y), _ptr(g), _ptr(beta), _ptr(out), T, D, C.c_float(1e-5), st)):
            rc = call()
            if rc != 0:
                raise RtError(rc, lib.rt_op_last_error().decode())
        torch.cuda.synchronize()
    return out.float()


def check_entry(entry, who, adapter, encoder=None):
    """dict(embeds=[E] | tokens=[t <= T, D] | image=<path | PIL image | [H, W, 3] uint8>, scale=float) -> a checked copy (tensors on the
    CPU, fp32; an image as the uint8 crop the encoder takes); ValueError otherwise.  `encoder`: the pipeline's image encoder or None.
    Under a plus adapter (adapter["resampler"]) an entry may be hidden=[N, E] - the encoder's penultimate hidden states -, and embeds= is
    refused: the pooled embedding is not the Resampler's input."""
    import torch
    plus = adapter.get("resampler") is not None
    if plus and isinstance(entry, dict) and sum(k in entry for k in ("embeds", "tokens", "image", "hidden")) == 1 and not set(entry) - {"embeds", "tokens", "image", "hidden", "scale"}:
        if "embeds" in entry:
            raise ValueError(f"{who}: embeds= is the pooled image embedding; the loaded adapter is a plus adapter, whose Resampler takes the encoder's "
                             f"penultimate hidden states: pass image=, hidden=[N, {adapter['E']}] or tokens=")
    elif not isinstance(entry, dict) or sum(k in entry for k in ("embeds", "tokens", "image")) != 1 or set(entry) - {"embeds", "tokens", "image", "scale"}:
        raise ValueError(f"{who}: expected dict(embeds=[E], tokens=[t, D] or image=picture, scale=number), got {entry!r}" if not isinstance(entry, dict)
                         else f"{who}: expected exactly one of embeds= / tokens= / image= and an optional scale=, got keys {sorted(entry)}")
    try:
        scale = float(entry.get("scale", 1.0))
    except (TypeError, ValueError):
        raise ValueError(f"{who}: scale must be a number, got {entry.get('scale')!r}")
    if not math.isfinite(scale):
        raise ValueError(f"{who}: scale must be finite, got {scale}")
    out = dict(scale=scale)
    if "image" in entry:
        if encoder is None:
            raise ValueError(f"{who}: image= needs an image encoder: none is loaded on this pipeline (load_image_encoder / --image_encoder)")
        if plus and getattr(encoder, "hidden_size", None) != adapter["E"]:
            raise ValueError(f"{who}: the image encoder's hidden_size is {getattr(encoder, 'hidden_size', None)}, the plus adapter's Resampler takes {adapter['E']}")
        if not plus and encoder.projection_dim != adapter["E"]:
            raise ValueError(f"{who}: the image encoder's projection_dim is {encoder.projection_dim}, the adapter's projection takes {adapter['E']}")
        from .clip_vision_encoder import preprocess
        try:
            out["image"] = torch.from_numpy(preprocess(entry["image"], encoder.S).copy())
        except ValueError as e:
            raise ValueError(f"{who}: {e}")
        return out
    if "embeds" in entry:
        e = torch.as_tensor(entry["embeds"]).detach().float().cpu().reshape(-1)
        if e.numel() != adapter["E"]:
            raise ValueError(f"{who}: embeds of {e.numel()} values: the adapter's projection takes {adapter['E']}")
        out["embeds"] = e
    elif "hidden" in entry:
        from .resampler import MAX_KEYS
        t = torch.as_tensor(entry["hidden"]).detach().float().cpu()
        if t.dim() != 2 or t.shape[0] < 1 or t.shape[0] + adapter["T"] > MAX_KEYS or t.shape[1] != adapter["E"]:
            raise ValueError(f"{who}: hidden must be [N <= {MAX_KEYS - adapter['T']}, {adapter['E']}], got {tuple(t.shape)}")
        out["hidden"] = t
    else:
        t = torch.as_tensor(entry["tokens"]).detach().float().cpu()
        if t.dim() != 2 or not 1 <= t.shape[0] <= adapter["T"] or t.shape[1] != adapter["D"]:
            raise ValueError(f"{who}: tokens must be [t <= {adapter['T']}, {adapter['D']}], got {tuple(t.shape)}")
        out["tokens"] = t
    if not bool(torch.isfinite(next(out[k] for k in ("embeds", "hidden", "tokens") if k in out)).all()):
        raise ValueError(f"{who}: non-finite values")
    return out


class IPAdapterMixin:
    """`load_ip_adapter(path)` / `unload_ip_adapter()` / `set_image_prompts(base=, regions=, negative=)` / `clear_image_prompts()` of a
    pipeline (and of HipUNet2DConditionModel, which holds the engines): the adapter and the image prompts are attributes, read by every
    sampling call right after it has set its text prompts (apply_image_prompts)."""
    ip_adapter = None        # what load_ip_adapter() of this module returns, or None
    image_encoder = None     # clip_vision_encoder.LazyImageEncoder / HipCLIPVisionEncoder (load_image_encoder), or None
    image_prompts = None     # dict(base=entry | None, regions={region index: entry}, negative=entry | None) or None

    def _ip_unet(self):
        return getattr(self, "unet", self)

    def load_ip_adapter(self, path_or_state_dict, dim_head=64):
        """`dim_head`: the head dim of a plus checkpoint's Resampler (its shapes do not tell it; 64 in every published one).  Engines are built with ip_tokens = T of this adapter from now on (existing ones are rebuilt on their next use).  On a rank
        whose UNet weights arrive by broadcast, load (or unload) BEFORE the first engine exists: afterwards the engines hold the only
        copy of the weights and install_ip_adapter refuses (RuntimeError)."""
        u = self._ip_unet()
        ad = load_ip_adapter(path_or_state_dict, u.config_dict, dim_head)
        u.install_ip_adapter(ad)                                     # (may refuse: nothing has changed then)
        self.ip_adapter, self.image_prompts = ad, None
        return self

    def unload_ip_adapter(self):
        self._ip_unet().install_ip_adapter(None)
        self.ip_adapter = self.image_prompts = None

    def load_image_encoder(self, path_or_encoder):
        """A CLIP vision encoder for `image=` entries: a directory in the Hugging Face layout (read and checked now, on the host; put on
        the GPU by the first image that needs it) or a HipCLIPVisionEncoder.  ValueError naming the file or key for anything unusable."""
        import os as _os
        if isinstance(path_or_encoder, (str, _os.PathLike)):
            from .clip_vision_encoder import LazyImageEncoder
            path_or_encoder = LazyImageEncoder(path_or_encoder)
        elif not (callable(path_or_encoder) and hasattr(path_or_encoder, "projection_dim") and hasattr(path_or_encoder, "S")):
            raise ValueError(f"load_image_encoder: expected a directory or a HipCLIPVisionEncoder, got {type(path_or_encoder).__name__}")
        self.image_encoder = path_or_encoder
        return self

    def unload_image_encoder(self):
        """Image prompts given as pictures keep what has been encoded already; new `image=` entries are refused again."""
        self.image_encoder = None

    def set_image_prompts(self, base=None, regions=None, negative=None):
        """Each entry: dict(embeds=[E] | tokens=[t <= T, D] | image=picture (needs load_image_encoder), scale=float); under a plus adapter
        dict(image= | hidden=[N, E] | tokens=, scale=).  `base`: the base prompt, in the plain AND the rich pass;
        `regions`: {index of a region prompt in the rich pass's prompt list: entry}; `negative` (default none): the unconditional stream
        then stays text-only, so guidance amplifies the image like the text - the projection of a zero embedding there reproduces
        diffusers' single-image behaviour."""
        if self.ip_adapter is None:
            raise ValueError("set_image_prompts: no IP-Adapter loaded (load_ip_adapter first)")
        who = f"{type(self).__name__}.set_image_prompts"
        if regions is not None and not isinstance(regions, dict):
            raise ValueError(f"{who}: regions must be a dict {{region index: entry}}, got {type(regions).__name__}")
        reg = {}
        for k, v in (regions or {}).items():
            if isinstance(k, bool) or not isinstance(k, int) or k < 0:
                raise ValueError(f"{who}: region index must be an integer >= 0, got {k!r}")
            reg[k] = check_entry(v, f"{who}: regions[{k}]", self.ip_adapter, self.image_encoder)
        ip = dict(base=check_entry(base, f"{who}: base", self.ip_adapter, self.image_encoder) if base is not None else None, regions=reg,
                  negative=check_entry(negative, f"{who}: negative", self.ip_adapter, self.image_encoder) if negative is not None else None)
        self.image_prompts = ip if (ip["base"] or ip["regions"] or ip["negative"]) else None

    def clear_image_prompts(self):
        self.image_prompts = None

    def image_prompt_slots(self, n_prompts, rich):
        """The image prompts per prompt slot of a call that sets n_prompts prompts - [negative, base] (plain pass) or [negative, region
        prompts ..., base] (rich pass) -: {slot: entry} or None.  A region index beyond the request's regions is a ValueError - raised
        here, before anything is launched."""
        ip = self.image_prompts
        if ip is None or self.ip_adapter is None:
            return None
        slots = {}
        if ip["negative"] is not None:
            slots[0] = ip["negative"]
        if ip["base"] is not None:
            slots[n_prompts - 1] = ip["base"]
        if rich:
            n_regions = n_prompts - 2
            for k, e in ip["regions"].items():
                if k >= n_regions:
                    raise ValueError(f"image prompt for region {k}: the request has {n_regions} region prompt(s)")
                slots[k + 1] = e
        return slots

    def apply_image_prompts(self, eng, slots, n_prompts):
        """Right after eng.set_prompts (which switched every image off): the tokens, counts and scales of `slots` onto `eng`."""
        if not slots:
            return
        import torch
        ad = self.ip_adapter
        T, D = ad["T"], ad["D"]
        dev = f"cuda:{eng.device}"
        tokens = torch.zeros(n_prompts, T, D, device=dev)
        counts, scales = [T] * n_prompts, [0.0] * n_prompts
        for s, e in slots.items():
            if ad.get("resampler") is not None:                      # a plus adapter: penultimate hidden states -> Resampler -> tokens
                if "image" in e and "_hidden" not in e:              # encoded once per picture, outside the step
                    enc = self.image_encoder
                    if enc is None:
                        raise ValueError("image prompt given as a picture: the image encoder was unloaded before it was encoded")
                    enc = enc.on(eng.device) if hasattr(enc, "on") else enc
                    e["_hidden"] = enc(e["image"][None], output_hidden_states=True).hidden_states[-2][0].float().cpu()
                if "_tokens" not in e:                               # resampled once per image, outside the step
                    e["_tokens"] = e["tokens"] if "tokens" in e else resample(ad, e["_hidden"] if "image" in e else e["hidden"], eng.device).cpu()
            if "image" in e and "_embeds" not in e and "_tokens" not in e:   # encoded once per picture, outside the step
                enc = self.image_encoder
                if enc is None:
                    raise ValueError("image prompt given as a picture: the image encoder was unloaded before it was encoded")
                enc = enc.on(eng.device) if hasattr(enc, "on") else enc
                e["_embeds"] = enc(e["image"][None]).image_embeds[0].float().cpu()
            if "_tokens" not in e:                                   # projected once per image, outside the step
                e["_tokens"] = project(ad, e["_embeds"] if "image" in e else e["embeds"], eng.device).cpu() if "tokens" not in e else e["tokens"]
            t = e["_tokens"]
            tokens[s, :t.shape[0]] = t.to(dev)
            counts[s], scales[s] = int(t.shape[0]), e["scale"]
        eng.set_image_prompts(tokens, scales, counts)


# ---------------------------------------------------------------------------------------------------------------- command line
def _parse_spec(spec, who, suffixes, fold_case=False):
    parts = str(spec).split(":")
    if not parts[0] or len(parts) > 3:
        raise ValueError(f"{who}: expected FILE[:TARGET[:SCALE]], got {spec!r}")
    target = parts[1] if len(parts) > 1 and parts[1] != "" else "base"
    if target not in ("base", "negative"):
        if not target.isdigit():
            raise ValueError(f"{who}: TARGET must be base, negative or a region number, got {target!r}")
        target = int(target)
    try:
        scale = float(parts[2]) if len(parts) > 2 else 1.0
    except ValueError:
        raise ValueError(f"{who}: SCALE must be a number, got {parts[2]!r}")
    if not math.isfinite(scale):
        raise ValueError(f"{who}: SCALE must be finite, got {parts[2]!r}")
    ext = os.path.splitext(parts[0])[1]
    if not (ext.lower() if fold_case else ext) in suffixes:
        raise ValueError(f"{who}: the file must be {', '.join(suffixes[:-1])} or {suffixes[-1]}, got {parts[0]!r}")
    return parts[0], target, scale


def parse_embeds_arg(spec, who="--ip_image_embeds"):
    """FILE[:TARGET[:SCALE]] -> (file, target, scale): TARGET is base (default), negative or a region number, SCALE a finite number
    (default 1).  ValueError otherwise."""
    return _parse_spec(spec, who, (".pt", ".npy", ".safetensors"))


IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".webp", ".bmp")


def parse_image_arg(spec, who="--ip_images"):
    """FILE[:TARGET[:SCALE]] for a picture (.png, .jpg, ...) -> (file, target, scale), parse_embeds_arg's grammar.  ValueError otherwise."""
    return _parse_spec(spec, who, IMAGE_SUFFIXES, fold_case=True)


def read_embeds(path):
    """An image embedding from a .pt (tensor, or a dict with one), .npy or .safetensors (its only tensor, or the one named image_embeds)."""
    import torch
    if not os.path.isfile(path):
        raise ValueError(f"image embedding file not found: {path}")
    if path.endswith(".npy"):
        import numpy as np
        return torch.from_numpy(np.load(path)).float()
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        d = load_file(path)
    else:
        d = torch.load(path, map_location="cpu", weights_only=True)
    if isinstance(d, dict):
        if "image_embeds" in d:
            d = d["image_embeds"]
        elif len(d) == 1:
            d = next(iter(d.values()))
        else:
            raise ValueError(f"{path}: holds {len(d)} tensors and none is named image_embeds")
    return torch.as_tensor(d).float()


def image_prompts_from_specs(specs, who="--ip_image_embeds", images=None, who_images="--ip_images"):
    """A list of FILE[:TARGET[:SCALE]] (or of dicts {"file", "target", "scale"} as a --requests line carries them) -> the keyword
    arguments of set_image_prompts, the files not read yet: dict(base=, regions=, negative=) with entries dict(file=, scale=).
    `specs` may also be the object form {"embeds": [...], "images": [...]} of a --requests line; `images`: the same list grammar for
    pictures (parse_image_arg), entries dict(image_file=, scale=).  Two prompts for one target are an error, whichever kind they are."""
    if isinstance(specs, dict):
        if set(specs) - {"embeds", "images"}:
            raise ValueError(f"{who}: expected a list or {{\"embeds\": [...], \"images\": [...]}}, got keys {sorted(specs)}")
        return image_prompts_from_specs(specs.get("embeds"), who, specs.get("images"), who + ": images")
    out = dict(base=None, regions={}, negative=None)
    for spec in images or []:
        if isinstance(spec, dict):
            if "file" not in spec or set(spec) - {"file", "target", "scale"}:
                raise ValueError(f"{who_images}: expected {{\"file\": ..., \"target\": ..., \"scale\": ...}}, got {spec!r}")
            spec = ":".join(str(spec.get(k, d)) for k, d in (("file", ""), ("target", "base"), ("scale", 1.0)))
        f, target, scale = parse_image_arg(spec, who_images)
        if (out["regions"].get(target) if isinstance(target, int) else out[target]) is not None:
            raise ValueError(f"{who_images}: two image prompts for target {target}")
        if isinstance(target, int):
            out["regions"][target] = dict(image_file=f, scale=scale)
        else:
            out[target] = dict(image_file=f, scale=scale)
    for spec in specs or []:
        if isinstance(spec, dict):
            if "file" not in spec or set(spec) - {"file", "target", "scale"}:
                raise ValueError(f"{who}: expected {{\"file\": ..., \"target\": ..., \"scale\": ...}}, got {spec!r}")
            spec = ":".join(str(spec.get(k, d)) for k, d in (("file", ""), ("target", "base"), ("scale", 1.0)))
        f, target, scale = parse_embeds_arg(spec, who)
        entry = dict(file=f, scale=scale)
        taken = out["regions"].get(target) if isinstance(target, int) else out[target]
        if taken is not None:
            raise ValueError(f"{who}: two image prompts for target {target}")
        if isinstance(target, int):
            out["regions"][target] = entry
        else:
            out[target] = entry
    return out


def apply_specs(model, parsed):
    """set_image_prompts on `model` from image_prompts_from_specs' result (reads the files); nothing parsed = clear.  ValueError when
    there are image prompts and `model` has no adapter loaded."""
    if parsed is not None and (parsed["base"] or parsed["regions"] or parsed["negative"]) and getattr(model, "ip_adapter", None) is None:
        raise ValueError("image prompts need an IP-Adapter: none is loaded on this pipeline (load_ip_adapter / --ip_adapter)")
    def entry(e):
        if e is None:
            return None
        if "image_file" in e:                                         # a picture: the pipeline's image encoder turns it into the embedding
            return dict(image=e["image_file"], scale=e["scale"])
        t = read_embeds(e["file"])
        while t.dim() > 2 or (t.dim() == 2 and t.shape[0] == 1 and t.numel() == model.ip_adapter["E"] and model.ip_adapter.get("resampler") is None):
            t = t[0]                                                  # a leading batch dimension of one
        # a [t, D] matrix = ready tokens (a Resampler's output, say); anything else = one image embedding - or, under a plus adapter, any
        # other matrix = the encoder's hidden states [N, E]
        ad = model.ip_adapter
        if t.dim() == 2 and ad.get("resampler") is not None and not (t.shape[0] <= ad["T"] and t.shape[1] == ad["D"]):
            return dict(hidden=t, scale=e["scale"])
        return dict(tokens=t, scale=e["scale"]) if t.dim() == 2 else dict(embeds=t, scale=e["scale"])
    if parsed is None or not (parsed["base"] or parsed["regions"] or parsed["negative"]):
        model.clear_image_prompts()
        return
    model.set_image_prompts(base=entry(parsed["base"]), regions={k: entry(v) for k, v in parsed["regions"].items()}, negative=entry(parsed["negative"]))
