"""Perturbed-attention guidance (Ahn et al. 2024: "Self-Rectifying Diffusion Sampling with Perturbed-Attention Guidance"), scaled per prompt
slot.  A slot with sigma != 0 gets a TWIN of its conditional stream in the step's one batched forward; at the applied attn1 modules the
twin's self-attention is the identity (its attention output is its V), and its prediction P is pushed away from:

    eps = u + g (sum_r m_r T_r - u) + sum_r m_r sigma_r (T_r - P_r)

The arithmetic runs inside the engine (csrc/pag.hip, include/rtdiff.h: rt_set_pag_layers / rt_set_pag_scales); this module holds the host
side: the layer specs, the slot-scale vector, the pipeline attribute both facades share and the command-line forms.

sigma is per prompt slot - base, each rich-text region; the negative prompt has no twin - so a request can firm up the structure of one
region and leave another alone.  A slot with sigma 0 runs nothing and keeps its bits.

The semantics are diffusers' enable_pag / pag_scale / pag_applied_layers with PAGCFGIdentitySelfAttnProcessor2_0 as remembered: diffusers
is not a dependency, so parity with it is unpinned; tests/pag_ref.py pins the restatement.

Not here: pag_adaptive_scale and a start / end window, PAG without classifier-free guidance, the Gaussian-blur variant (SAG), PAG together
with guidance_rescale, perturbing the ControlNet copy, the operator seams HipAttnProcessor / HipUNet2DConditionModel.__call__."""
import math
import re

DEFAULT_LAYERS = ("mid",)
_BLOCK = re.compile(r"^(down_blocks|up_blocks)\.(\d+)(?:\.attentions\.(\d+))?$")
_MID = re.compile(r"^mid_block(?:\.attentions\.(\d+))?$")


_FULL = re.compile(r"^(mid_block|(down_blocks|up_blocks)\.\d+)\.attentions\.\d+\.transformer_blocks\.\d+\.attn([12])$")


def check_layer_forms(specs):
    """The FORM of every layer spec, for callers that do not know the UNet yet (the command line, before any rank starts): mid, down, up,
    down_blocks.N, up_blocks.N, mid_block, ...attentions.M, or a full module name <block>.attentions.M.transformer_blocks.K.attn1 with any
    M and K.  Whether the UNet has such a module is resolve_layers' question.  ValueError naming the offender."""
    if isinstance(specs, str):
        specs = (specs,)
    for spec in specs:
        if not isinstance(spec, str) or not spec:
            raise ValueError(f"pag layers: a layer spec must be a non-empty string, got {spec!r}")
        full = _FULL.match(spec)
        if full and full.group(3) == "2":
            raise ValueError(f"pag layers: {spec} is a cross-attention module; perturbed attention applies to attn1 modules only")
        if not (full or spec in ("mid", "down", "up") or _BLOCK.match(spec) or _MID.match(spec)):
            raise ValueError(f"pag layers: unknown layer spec {spec!r} (mid, down, up, down_blocks.N, up_blocks.N, ...attentions.M or a full attn1 module name)")


def attn1_names(modules):
    """The attn1 module names among `modules`: names, or Engine.attn_modules()'s (name, max tokens, heads) entries, in their order."""
    names = [m if isinstance(m, str) else m[0] for m in modules]
    return [n for n in names if n.endswith(".attn1")]


def resolve_layers(specs, modules):
    """Layer specs -> the full attn1 module names they cover, in `modules`' (execution) order, each once.  A spec is `mid`, `down`, `up`,
    `down_blocks.N`, `up_blocks.N`, `mid_block`, any of those followed by `.attentions.M`, or a full attn1 module name.  ValueError naming
    the offender for an unknown form, a spec that covers no module, or an attn2 name."""
    if isinstance(specs, str):
        specs = (specs,)
    every = [m if isinstance(m, str) else m[0] for m in modules]
    a1 = attn1_names(every)
    picked = set()
    for spec in specs:
        if not isinstance(spec, str) or not spec:
            raise ValueError(f"pag layers: a layer spec must be a non-empty string, got {spec!r}")
        if spec.endswith(".attn2") and spec in every:
            raise ValueError(f"pag layers: {spec} is a cross-attention module; perturbed attention applies to attn1 modules only")
        if spec in a1:
            picked.add(spec)
            continue
        if spec in ("mid", "down", "up"):
            prefix = {"mid": "mid_block.", "down": "down_blocks.", "up": "up_blocks."}[spec]
        elif _BLOCK.match(spec) or _MID.match(spec):
            prefix = spec + "."
        else:
            raise ValueError(f"pag layers: unknown layer spec {spec!r} (mid, down, up, down_blocks.N, up_blocks.N, ...attentions.M or a full attn1 module name)")
        hit = [n for n in a1 if n.startswith(prefix)]
        if not hit:
            raise ValueError(f"pag layers: {spec!r} covers no self-attention module of this UNet")
        picked.update(hit)
    return [n for n in a1 if n in picked]


def _number(v, who):
    try:
        f = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{who} must be a number, got {v!r}")
    if isinstance(v, bool) or not math.isfinite(f):
        raise ValueError(f"{who} must be a finite number, got {v!r}")
    return f


def slot_scales(pag, n_prompts, rich):
    """The sigma of every prompt slot of a call that sets n_prompts prompts - [negative, text] (plain pass) or [negative, region prompts
    ..., base] (rich pass) - from a request dict(scale=, regions={i: s}, base=): `base` (default: scale) for the base / text slot, `scale`
    for every region unless regions[i] overrides it, 0 for the negative slot, which has no twin.  A region index beyond the request's
    regions is a ValueError."""
    out = [0.0] * n_prompts
    base = pag["scale"] if pag.get("base") is None else pag["base"]
    out[n_prompts - 1] = base
    n_regions = n_prompts - 2
    if rich:
        for r in range(n_regions):
            out[r + 1] = pag["scale"]
        for k, s in pag["regions"].items():
            if k >= n_regions:
                raise ValueError(f"pag scale for region {k}: the request has {n_regions} region prompt(s)")
            out[k + 1] = s
    return out


def twin_count(scales, rich, use_ref=True):
    """An upper bound of the twin streams a step adds for the slot scales: one per conditional slot with sigma != 0, and text_ref's while
    the reference pair may be stepped."""
    if scales is None:
        return 0
    n = sum(1 for s in scales[1:] if s != 0.0)
    if rich and use_ref and scales[-1] != 0.0:
        n += 1
    return n


def check_guidance(scales, guidance_scale, guidance_rescale, who="pag"):
    """The two refused combinations, before anything is launched (the engine refuses them too)."""
    if scales is None or all(s == 0.0 for s in scales):
        return
    if float(guidance_scale) == 0.0:
        raise ValueError(f"{who}: perturbed-attention guidance needs classifier-free guidance: guidance_scale is 0")
    if float(guidance_rescale or 0.0) > 0.0:
        raise ValueError(f"{who}: perturbed-attention guidance together with guidance_rescale > 0 is not supported")


class PagMixin:
    """`set_pag(scale=3.0, regions={i: s}, base=None, layers=("mid",))` / `clear_pag()` of a pipeline (and of HipUNet2DConditionModel): the
    request is an attribute, read by every sampling call right after it has set its text prompts (apply_pag)."""
    pag = None               # dict(scale=, regions=, base=, layers=) or None

    def set_pag(self, scale=3.0, regions=None, base=None, layers=DEFAULT_LAYERS):
        """`scale`: the default sigma of the base prompt and of every rich-text region; `base=` overrides it for the base prompt (the text
        prompt of the plain pass), `regions={i: s}` for region i.  `layers`: the applied self-attention modules (resolve_layers)."""
        who = f"{type(self).__name__}.set_pag"
        if regions is not None and not isinstance(regions, dict):
            raise ValueError(f"{who}: regions must be a dict {{region index: scale}}, got {type(regions).__name__}")
        reg = {}
        for k, v in (regions or {}).items():
            if isinstance(k, bool) or not isinstance(k, int) or k < 0:
                raise ValueError(f"{who}: region index must be an integer >= 0, got {k!r}")
            reg[k] = _number(v, f"{who}: regions[{k}]")
        if isinstance(layers, str):
            layers = (layers,)
        layers = tuple(layers)
        if not layers or not all(isinstance(s, str) and s for s in layers):
            raise ValueError(f"{who}: layers must be a non-empty sequence of layer specs, got {layers!r}")
        self.pag = dict(scale=_number(scale, f"{who}: scale"), regions=reg, base=None if base is None else _number(base, f"{who}: base"), layers=layers)

    def clear_pag(self):
        self.pag = None

    def _pag_request(self):
        """The pipeline's own request, else its UNet's (HipUNet2DConditionModel.set_pag), as with FreeU."""
        if self.pag is not None:
            return self.pag
        return getattr(getattr(self, "unet", None), "pag", None)

    def pag_slot_scales(self, n_prompts, rich, guidance_scale=None, guidance_rescale=0.0):
        """The sigma of every prompt slot of the call, or None without a request; the refused combinations raise here, before any launch."""
        pag = self._pag_request()
        if pag is None:
            return None
        scales = slot_scales(pag, n_prompts, rich)
        if guidance_scale is not None:
            check_guidance(scales, guidance_scale, guidance_rescale, f"{type(self).__name__}")
        return scales

    def apply_pag(self, eng, scales):
        """Right after eng.set_prompts (which reset every sigma): the applied layers and the slot scales onto `eng`."""
        if scales is None or all(s == 0.0 for s in scales):
            return
        eng.set_pag_layers(resolve_layers(self._pag_request()["layers"], eng.attn_modules()))
        eng.set_pag_scales(scales)


# ---------------------------------------------------------------------------------------------------------------- command line
def parse_scale_args(values, who="--pag_scale"):
    """['S', 'TARGET:S', ...] (or one string / number) -> dict(scale=, regions={i: s}, base=), the scale arguments of set_pag: a bare S is the
    default of the base prompt and every region, TARGET is base or a region number.  ValueError otherwise."""
    if isinstance(values, (str, int, float)):
        values = [values]
    out = dict(scale=None, regions={}, base=None)
    for v in values or []:
        s = str(v)
        target, sep, num = s.rpartition(":")
        if sep and target != "base" and not target.isdigit():
            raise ValueError(f"{who}: TARGET must be base or a region number, got {target!r} in {s!r}")
        try:
            f = float(num)
        except ValueError:
            raise ValueError(f"{who}: S must be a number, got {num!r} in {s!r}")
        if not math.isfinite(f):
            raise ValueError(f"{who}: S must be finite, got {num!r}")
        if not sep:
            if out["scale"] is not None:
                raise ValueError(f"{who}: two default scales ({out['scale']} and {f})")
            out["scale"] = f
        elif target == "base":
            if out["base"] is not None:
                raise ValueError(f"{who}: two scales for base")
            out["base"] = f
        else:
            if int(target) in out["regions"]:
                raise ValueError(f"{who}: two scales for region {target}")
            out["regions"][int(target)] = f
    if out["scale"] is None:
        out["scale"] = 0.0 if (out["regions"] or out["base"] is not None) else 3.0
    return out


def pag_from_request(obj, who="pag"):
    """A --requests line's "pag": S | [S, "TARGET:S", ...] | {"scale": ..., "layers": [SPEC, ...]} -> set_pag's keyword arguments."""
    layers = DEFAULT_LAYERS
    if isinstance(obj, dict):
        if set(obj) - {"scale", "layers"}:
            raise ValueError(f"{who}: expected {{\"scale\": ..., \"layers\": [...]}}, got {obj!r}")
        layers = obj.get("layers", DEFAULT_LAYERS)
        obj = obj.get("scale", 3.0)
    if isinstance(obj, bool) or not isinstance(obj, (int, float, str, list, tuple)):
        raise ValueError(f"{who}: expected a scale, a list of scales or a dict, got {obj!r}")
    kw = parse_scale_args(list(obj) if isinstance(obj, (list, tuple)) else obj, f"{who}: scale")
    if isinstance(layers, str):
        layers = (layers,)
    if not isinstance(layers, (list, tuple)) or not layers or not all(isinstance(s, str) and s for s in layers):
        raise ValueError(f"{who}: layers must be a non-empty list of layer specs, got {layers!r}")
    kw["layers"] = tuple(layers)
    return kw


def expected_streams(R, scales, inject, step_ref, run_ref=True):
    """The stream list of a rich step with R masks (R - 1 region prompts) as the engine plans it, as labels: [uncond, base, uncond_ref,
    text_ref, region 0 .., twin of base, twin of text_ref (while the pair is stepped), twins of the regions with sigma != 0].  `scales`:
    the slot vector [negative, regions ..., base] or None.  Host-side restatement of region_plan for tests and tools."""
    out = ["uncond", "base"]
    if run_ref:
        out += ["uncond_ref", "text_ref"]
    out += [f"region{r}" + ("<-text_ref" if inject and run_ref else "") for r in range(R - 1)]
    if scales is not None and any(s != 0.0 for s in scales):
        if scales[R] != 0.0:
            out.append("twin(base)")
            if run_ref and step_ref:
                out.append("twin(text_ref)")
        out += [f"twin(region{r})" for r in range(R - 1) if scales[r + 1] != 0.0]
    return out
