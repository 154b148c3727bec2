"""ControlNet (Zhang et al. 2023: "Adding Conditional Control to Text-to-Image Diffusion Models"): a second copy of the UNet's encoder reads
the latents plus an embedded hint image (edges, depth, pose, a scribble) and adds, through one 1x1 "zero convolution" per skip connection
and one behind the mid block, residuals to the main UNet's skips and mid output.  The layer arithmetic runs inside the engine
(csrc/control.hip, include/rtdiff.h: rt_set_control_hint / rt_set_control_scales); this module holds the host side: the checkpoint loader,
the hint's preprocessing and the pipeline attribute both facades share.

The hint is one image for the whole picture; its SCALE is per prompt slot - base, each rich-text region, negative - so a request can hold
one region tightly to the hint and leave another free.  A stream whose slot has scale 0 does not run the control copy and keeps its bits.

The formulas and key names are diffusers' ControlNetModel as remembered: diffusers is not a dependency, so parity with it is unpinned;
tests/controlnet_ref.py pins the restatement.

Not here: several ControlNets at once, guess mode / global_pool_conditions, T2I-Adapter, reference-only control, ControlNet-XS and LoRA-form
ControlNets, a hint per region, hint preprocessors (Canny and the like), the operator seams HipAttnProcessor / HipUNet2DConditionModel.__call__."""
import json
import math
import os

PREFIX = "controlnet."
_CE = "controlnet_cond_embedding."


def _read(path):
    """A .safetensors / .bin file, or a directory in diffusers' layout (config.json + diffusion_pytorch_model.*) -> (state dict, config or {})."""
    cfg = {}
    if os.path.isdir(path):
        cj = os.path.join(path, "config.json")
        if os.path.isfile(cj):
            with open(cj) as f:
                cfg = json.load(f)
        cand = [os.path.join(path, n) for n in ("diffusion_pytorch_model.safetensors", "diffusion_pytorch_model.bin")]
        path = next((c for c in cand if os.path.isfile(c)), None)
        if path is None:
            raise ValueError(f"ControlNet: no diffusion_pytorch_model.safetensors / .bin in {os.path.dirname(cand[0])}")
    if not os.path.isfile(path):
        raise ValueError(f"ControlNet checkpoint not found: {path}")
    if path.endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(path), cfg
    import torch
    return torch.load(path, map_location="cpu", weights_only=True), cfg


def expected_weights(config, embed_channels, hint_channels=3):
    """{checkpoint key: shape} of the ControlNet of UNet `config`: the engine's own weight table (a weight-table-only engine: no device
    needed), the names under its "controlnet." prefix."""
    from .engine import Engine
    e = Engine(config, 8, 8, device=-1, controlnet=dict(embed_channels=tuple(embed_channels), hint_channels=hint_channels))
    try:
        return {n[len(PREFIX):]: s for n, s in e.weight_table() if n.startswith(PREFIX)}
    finally:
        e.close()


def load_controlnet(path_or_state_dict, config, guess_mode=False, global_pool_conditions=False):
    """A ControlNet checkpoint in diffusers' ControlNetModel layout for the UNet `config` -> dict(weights = {"controlnet.<key>": tensor} under
    the engine's names, embed_channels = the four stage widths of the hint embedder (from the shapes), hint_channels).  ValueError naming
    the key for: a missing or left-over key, an encoder shape that does not match the UNet, `class_embedding.*` (class-conditioned
    ControlNets), and for a guess_mode / global_pool_conditions request (the argument, or the checkpoint directory's config.json)."""
    ck_cfg = {}
    if isinstance(path_or_state_dict, (str, os.PathLike)):
        sd, ck_cfg = _read(str(path_or_state_dict))
    else:
        sd = path_or_state_dict
    sd = dict(sd)
    if guess_mode:
        raise ValueError("ControlNet: guess_mode is not supported (the residuals are scaled per prompt slot, not per depth)")
    if global_pool_conditions or ck_cfg.get("global_pool_conditions"):
        raise ValueError("ControlNet: global_pool_conditions is not supported (the residuals are added per pixel)")
    for k in sd:
        if k.startswith("class_embedding."):
            raise ValueError(f"ControlNet: {k}: class-conditioned ControlNets (class_embedding) are not supported")
    ch = []
    for k in (_CE + "conv_in.weight", _CE + "blocks.1.weight", _CE + "blocks.3.weight", _CE + "blocks.5.weight"):
        if k not in sd:
            raise ValueError(f"ControlNet: missing key {k}")
        if sd[k].dim() != 4 or tuple(sd[k].shape[2:]) != (3, 3):
            raise ValueError(f"ControlNet: {k} has shape {tuple(sd[k].shape)}: expected a 3x3 convolution")
        ch.append(int(sd[k].shape[0]))
    hint_channels = int(sd[_CE + "conv_in.weight"].shape[1])
    if any(c < 8 or c % 8 for c in ch):
        raise ValueError(f"ControlNet: the hint embedder's channels {tuple(ch)} must be multiples of 8")
    want = expected_weights(config, ch, hint_channels)
    weights = {}
    for k, shape in want.items():
        if k not in sd:
            raise ValueError(f"ControlNet: missing key {k}")
        t = sd.pop(k)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"ControlNet: {k} has shape {tuple(t.shape)}, the UNet's config needs {tuple(shape)}: the checkpoint does not belong to this UNet")
        weights[PREFIX + k] = t
    if sd:
        raise ValueError(f"ControlNet: left-over key {sorted(sd)[0]} ({len(sd)} in all): the checkpoint does not belong to this UNet")
    return dict(weights=weights, embed_channels=tuple(ch), hint_channels=hint_channels)


def preprocess_hint(image, height, width):
    """A path, a PIL image or an [H, W, 3] uint8 array -> fp32 numpy [3, height, width] in 0 .. 1, resized to height x width (bicubic, as
    PIL does it; an image that already has the size is only converted).  height / width must be multiples of 8.  ValueError otherwise."""
    import numpy as np
    from PIL import Image
    if height < 8 or width < 8 or height % 8 or width % 8:
        raise ValueError(f"control image: height and width must be multiples of 8, got {height} x {width}")
    if isinstance(image, (str, os.PathLike)):
        if not os.path.isfile(image):
            raise ValueError(f"control image not found: {image}")
        image = Image.open(image)
    if isinstance(image, Image.Image):
        img = image.convert("RGB")
    else:
        a = np.asarray(image)
        if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3:
            raise ValueError(f"control image: expected a path, a PIL image or an [H, W, 3] uint8 array, got {getattr(a, 'dtype', None)} {getattr(a, 'shape', None)}")
        img = Image.fromarray(a)
    if img.size != (width, height):
        img = img.resize((width, height), Image.BICUBIC)
    return np.ascontiguousarray(np.asarray(img, dtype=np.uint8).transpose(2, 0, 1).astype(np.float32) / 255.0)


def control_window(n_steps, start, end):
    """The steps of an executed schedule of n_steps that are controlled, as diffusers' control_guidance_start / _end decide it: step i is
    controlled unless i / n < start or (i + 1) / n > end."""
    return [i for i in range(n_steps) if not (i / n_steps < start or (i + 1) / n_steps > end)]


def _number(v, who):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{who} must be a number, got {v!r}")
    if isinstance(v, bool) or not math.isfinite(f):
        raise ValueError(f"{who} must be a finite number, got {v!r}")
    return f


class ControlNetMixin:
    """`load_controlnet(path)` / `unload_controlnet()` / `set_control(image=, scale=, regions=, negative=, start=, end=)` / `clear_control()`
    of a pipeline (and of HipUNet2DConditionModel, which holds the engines): the ControlNet and the control request are attributes, read by
    every sampling call right after it has set its text prompts (apply_control) and by the step loops (denoise_loop), which switch the
    scales on and off at the window's boundaries, between steps."""
    controlnet = None        # what load_controlnet() of this module returns, or None
    control = None           # dict(image=, scale=, regions=, negative=, start=, end=) or None

    def _cn_unet(self):
        return getattr(self, "unet", self)

    def load_controlnet(self, path_or_state_dict):
        """Engines are built with the ControlNet from now on (existing ones are rebuilt on their next use).  On a rank whose UNet weights
        arrive by broadcast, load (or unload) BEFORE the first engine exists (install_controlnet refuses afterwards)."""
        u = self._cn_unet()
        cn = load_controlnet(path_or_state_dict, u.config_dict)
        u.install_controlnet(cn)
        self.controlnet, self.control = cn, None
        return self

    def unload_controlnet(self):
        self._cn_unet().install_controlnet(None)
        self.controlnet = self.control = None

    def set_control(self, image=None, scale=1.0, regions=None, negative=None, start=0.0, end=1.0):
        """`image`: the hint - a path, a PIL image, an [H, W, 3] uint8 array (resized to the request's size) or a float tensor / array
        [hint_channels, H, W] with the values the checkpoint expects (taken as is: H, W must be the request's size).  `scale`: the default of
        every prompt slot - as in diffusers the unconditional half is controlled too; `negative=` overrides it for the negative prompt,
        `regions={i: s}` for rich-text region i.  `start` / `end`: the controlled fraction of the executed schedule (diffusers'
        control_guidance_start / control_guidance_end), in both passes."""
        who = f"{type(self).__name__}.set_control"
        if self.controlnet is None:
            raise ValueError(f"{who}: no ControlNet loaded (load_controlnet first)")
        if image is None:
            raise ValueError(f"{who}: image= is required")
        if regions is not None and not isinstance(regions, dict):
            raise ValueError(f"{who}: regions must be a dict {{region index: scale}}, got {type(regions).__name__}")
        reg = {}
        for k, v in (regions or {}).items():
            if isinstance(k, bool) or not isinstance(k, int) or k < 0:
                raise ValueError(f"{who}: region index must be an integer >= 0, got {k!r}")
            reg[k] = _number(v, f"{who}: regions[{k}]")
        start, end = _number(start, f"{who}: start"), _number(end, f"{who}: end")
        if not (0.0 <= start <= 1.0 and 0.0 <= end <= 1.0 and start < end):
            raise ValueError(f"{who}: need 0 <= start < end <= 1, got start {start}, end {end}")
        self.control = dict(image=image, scale=_number(scale, f"{who}: scale"), regions=reg,
                            negative=None if negative is None else _number(negative, f"{who}: negative"), start=start, end=end)

    def clear_control(self):
        self.control = None

    def control_scales(self, n_prompts, rich):
        """The scale of every prompt slot of a call that sets n_prompts prompts - [negative, base] (plain pass) or [negative, region prompts
        ..., base] (rich pass) -, or None without a control request.  A region index beyond the request's regions is a ValueError - raised
        here, before anything is launched."""
        c = self.control
        if c is None or self.controlnet is None:
            return None
        scales = [c["scale"]] * n_prompts
        if c["negative"] is not None:
            scales[0] = c["negative"]
        n_regions = n_prompts - 2
        for k, s in c["regions"].items():
            if rich:
                if k >= n_regions:
                    raise ValueError(f"control scale for region {k}: the request has {n_regions} region prompt(s)")
                scales[k + 1] = s
        return scales

    def _hint_tensor(self, h, w):
        import numpy as np
        import torch
        img, hc = self.control["image"], self.controlnet["hint_channels"]
        if isinstance(img, torch.Tensor) and img.is_floating_point() or (isinstance(img, np.ndarray) and img.dtype.kind == "f"):
            t = torch.as_tensor(img).detach().float()
            t = t[0] if t.dim() == 4 and t.shape[0] == 1 else t
            if tuple(t.shape) != (hc, 8 * h, 8 * w):
                raise ValueError(f"control image: a float hint must be [{hc}, {8 * h}, {8 * w}] for this request, got {tuple(t.shape)}")
            return t
        if hc != 3:
            raise ValueError(f"control image: the loaded ControlNet takes {hc} hint channels: pass a float tensor [{hc}, H, W]")
        return torch.from_numpy(preprocess_hint(img, 8 * h, 8 * w))

    def apply_control(self, eng, scales, h, w):
        """Right after eng.set_prompts (which reset every scale): the hint onto `eng` (embedded once per call, outside the step) and the
        plan the step loops follow - pipe._control_run = (scales, controlled steps) or None."""
        self._control_run = None
        if scales is None:
            return
        if all(s == 0.0 for s in scales):
            return
        eng.set_control_hint(self._hint_tensor(h, w))
        self._control_run = (list(scales), set(control_window(len(self.scheduler.timesteps), self.control["start"], self.control["end"])))


def switch_control(pipe, eng, i):
    """Between steps (denoise_loop): the scales on at the first controlled step, off behind the last; nothing on a pipeline without control."""
    run = getattr(pipe, "_control_run", None)
    if run is None:
        return
    scales, steps = run
    on, was = i in steps, (i - 1) in steps and i > 0
    if on and not was:
        eng.set_control_scales(scales)
    elif was and not on:
        eng.set_control_scales([0.0] * len(scales))


# ---------------------------------------------------------------------------------------------------------------- command line
def parse_scale_args(values, who="--control_scale"):
    """['S', 'TARGET:S', ...] (or one string / number) -> dict(scale=, regions={i: s}, negative=), the scale arguments of set_control: a
    bare S is the default of every slot, TARGET is base, negative or a region number.  The base prompt has no entry of its own in
    set_control - it runs at the default - so `base:S` IS the bare S, and giving both is an error.  ValueError otherwise."""
    if isinstance(values, (str, int, float)):
        values = [values]
    out = dict(scale=None, regions={}, negative=None)
    for v in values or []:
        s = str(v)
        target, sep, num = s.rpartition(":")
        if not sep:
            target = "base"
        if target not in ("base", "negative") and not target.isdigit():
            raise ValueError(f"{who}: TARGET must be base, negative or a region number, got {target!r} in {s!r}")
        try:
            f = float(num)
        except ValueError:
            raise ValueError(f"{who}: S must be a number, got {num!r} in {s!r}")
        if not math.isfinite(f):
            raise ValueError(f"{who}: S must be finite, got {num!r}")
        if target == "base":
            if out["scale"] is not None:
                raise ValueError(f"{who}: two default scales ({out['scale']} and {f}): a bare S and base:S are the same entry")
            out["scale"] = f
        elif target == "negative":
            if out["negative"] is not None:
                raise ValueError(f"{who}: two scales for negative")
            out["negative"] = f
        else:
            if int(target) in out["regions"]:
                raise ValueError(f"{who}: two scales for region {target}")
            out["regions"][int(target)] = f
    if out["scale"] is None:
        out["scale"] = 1.0
    return out


def control_from_request(obj, who="control"):
    """A --requests line's "control": {"image": FILE, "scale": S | [S, "TARGET:S", ...], "start": a, "end": b} -> set_control's keyword
    arguments (the file not read yet).  ValueError otherwise."""
    if not isinstance(obj, dict) or "image" not in obj or set(obj) - {"image", "scale", "start", "end"}:
        raise ValueError(f"{who}: expected {{\"image\": FILE, \"scale\": ..., \"start\": ..., \"end\": ...}}, got {obj!r}")
    kw = parse_scale_args(obj.get("scale", 1.0), f"{who}: scale")
    kw.update(image=str(obj["image"]), start=_number(obj.get("start", 0.0), f"{who}: start"), end=_number(obj.get("end", 1.0), f"{who}: end"))
    return kw
