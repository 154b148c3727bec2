"""Regional LoRA: low-rank adapters kept UNMERGED and scaled per prompt slot, y = W x + s_slot (alpha / r) B (A x), so that one region can
be painted in watercolour and its neighbour in pixel art inside one forward (a merge - lora.py - gives every stream the same weights).

Host side of csrc/lora.hip (rt_op_lora_add).  Up to MAX_ADAPTERS adapters are resident; their factors are concatenated along the rank into
R <= MAX_RANK rank columns, every adapter's block zero-padded to the kernel's granule of 16 columns:

  down [R, K]   rows of adapter l at its block            up [N, R]   columns likewise
  alpha_over_rank [R]   alpha / rank of the module the column belongs to (0 on pad columns), PER MODULE as kohya checkpoints store it
  col_adapter [R]       the adapter a column belongs to (the same for every module: an adapter's block is as wide as its widest module)

and a stream's factor of column j is scale[slot][col_adapter[j]] * alpha_over_rank[j], kept in fp32 next to bf16 factors (never baked in).
Targets are the eight attention projections attn{1,2}.{to_q,to_k,to_v,to_out.0} of every BasicTransformerBlock - diffusers' LoRA training
targets; a tensor on any other module is refused by name (the merge, lora_path=, handles those) or dropped under attention_only=True.
targets="transformer" (opt-in) widens the set to every Linear / 1x1 convolution of Transformer2DModel - kohya's default network: also
ff.net.0.proj (csrc/lora.hip, rt_op_lora_geglu), ff.net.2, proj_in and proj_out; resnets, 3x3 convolutions, time_emb_proj and the
samplers stay refused.
Key layouts: lora.py's (kohya, diffusers 0.18, diffusers >= 0.20, peft)."""
import math
import re

import torch

from .lora import resolve_targets

MAX_ADAPTERS = 4
MAX_RANK = 128
GRANULE = 16                       # rank columns per MFMA tile of lora_add_kernel
PROJECTIONS = ("attn1.to_q", "attn1.to_k", "attn1.to_v", "attn1.to_out.0", "attn2.to_q", "attn2.to_k", "attn2.to_v", "attn2.to_out.0")
TRANSFORMER_MODULES = ("ff.net.0.proj", "ff.net.2", "proj_in", "proj_out")      # what targets="transformer" adds
TARGETS = ("attention", "transformer")
_TARGET = re.compile(r"\.transformer_blocks\.\d+\.attn[12]\.(to_q|to_k|to_v|to_out\.0)$")
_WIDE = re.compile(r"\.transformer_blocks\.\d+\.ff\.net\.(0\.proj|2)$|\.attentions\.\d+\.proj_(in|out)$")


def check_targets(targets):
    if targets not in TARGETS:
        raise ValueError(f"regional LoRA: targets must be one of {TARGETS}, got {targets!r}")
    return targets


def is_target(path, targets="attention"):
    return _TARGET.search(path) is not None or (targets == "transformer" and is_wide(path))


def is_wide(path):
    """One of the four modules targets="transformer" adds (an engine carries their slots only with lora_targets = 1)."""
    return _WIDE.search(path) is not None


def parse_adapter(unet_state_dict, lora_state_dict, attention_only=False, targets="attention"):
    """One checkpoint -> (modules, report): modules = module path -> (down [r, K] fp32, up [N, r] fp32, alpha), report = dict(applied=[paths],
    dropped=[paths] (attention_only), text_encoder=[keys], alpha_default=[paths]).  targets: "attention" = the eight attention projections,
    "transformer" = also ff.net.0.proj, ff.net.2, proj_in and proj_out (linear or 1x1 convolution)."""
    check_targets(targets)
    paths, groups, text_encoder = resolve_targets(unet_state_dict, lora_state_dict)
    other = sorted(p for p in groups if not is_target(p, targets))
    if other and not attention_only and targets == "transformer":
        raise ValueError(f"regional LoRA (targets=\"transformer\") applies to the attention projections {PROJECTIONS} and to {TRANSFORMER_MODULES} "
                         f"of a transformer; this checkpoint also adapts {other}: load it merged instead (lora_path=, lora_scale=), or pass "
                         "attention_only=True to drop those tensors")
    if other and not attention_only:
        raise ValueError(f"regional LoRA applies to the attention projections {PROJECTIONS} only; this checkpoint also adapts {other}: "
                         "load it merged instead (lora_path=, lora_scale=), or pass attention_only=True to drop those tensors "
                         "(targets=\"transformer\" also takes feed-forward, proj_in and proj_out adapters)")
    modules, report = {}, dict(applied=[], dropped=other, text_encoder=text_encoder, alpha_default=[])
    for path, g in groups.items():
        if path in other:
            continue
        if "down" not in g or "up" not in g:
            raise KeyError(f"LoRA pair for '{path}' is incomplete: {sorted(g)}")
        down, up = g["down"].float().flatten(1), g["up"].float().flatten(1)
        W = unet_state_dict[paths[path]]
        rank = down.shape[0]
        if up.shape != (W.shape[0], rank) or down.shape[1] != W.shape[1]:
            raise ValueError(f"LoRA factors {tuple(up.shape)} x {tuple(down.shape)} do not fit {paths[path]} {tuple(W.shape)}")
        if "alpha" in g:
            alpha = float(g["alpha"])
        else:
            alpha = float(rank); report["alpha_default"].append(path)
        modules[path] = (down, up, alpha)
        report["applied"].append(path)
    return modules, report


def pad_rank(r):
    return -(-r // GRANULE) * GRANULE


def rank_layout(adapters):
    """adapters: name -> modules (parse_adapter), in load order.  -> (names, width, first, R): adapter l owns rank columns
    first[l] .. first[l] + width[l] of every module, width = its widest module's rank padded to the granule."""
    names = list(adapters)
    if not 1 <= len(names) <= MAX_ADAPTERS:
        raise ValueError(f"{len(names)} regional adapters: between 1 and {MAX_ADAPTERS} can be resident")
    width = [pad_rank(max([m[0].shape[0] for m in adapters[n].values()] or [1])) for n in names]
    R = sum(width)
    if R > MAX_RANK:
        raise ValueError(f"the adapters' padded ranks {dict(zip(names, width))} add up to {R} rank columns; at most {MAX_RANK} fit")
    first = [sum(width[:l]) for l in range(len(names))]
    return names, width, first, R


def concat_module(adapters, path, K, N, layout=None):
    """The four tables of one module: (down [R, K], up [N, R], alpha_over_rank [R], col_adapter [R] int32), fp32.  An adapter that does
    not adapt `path` leaves its block zero."""
    names, width, first, R = layout or rank_layout(adapters)
    down, up = torch.zeros(R, K), torch.zeros(N, R)
    aor, col = torch.zeros(R), torch.zeros(R, dtype=torch.int32)
    for l, n in enumerate(names):
        col[first[l]:first[l] + width[l]] = l
        if path not in adapters[n]:
            continue
        d, u, alpha = adapters[n][path]
        r = d.shape[0]
        down[first[l]:first[l] + r] = d
        up[:, first[l]:first[l] + r] = u
        aor[first[l]:first[l] + r] = alpha / r
    return down, up, aor, col


def head_pad_rows(w, heads, d, DP):
    """[heads d, c] -> [heads DP, c], rows d .. DP of every head zero (the layout of the packed q / k / v projections)."""
    out = torch.zeros(heads, DP, w.shape[1], dtype=w.dtype)
    out[:, :d] = w.reshape(heads, d, -1)
    return out.reshape(heads * DP, -1)


def pack_module(down, up, projection, heads, d, DP):
    """The factors in the layout of the base weight they sit beside, bf16: `up` rows of to_q / to_k / to_v head-padded to DP (zero pad rows),
    to_q's times d^-1/2 log2 e (what the packed to_q carries); `down` columns of to_out.0 head-padded (zero pad columns)."""
    leaf = projection.split(".", 1)[1] if projection.startswith("attn") else projection
    if leaf == "to_out.0":
        down = head_pad_rows(down.t().contiguous(), heads, d, DP).t().contiguous()
    else:
        up = head_pad_rows(up, heads, d, DP)
        if leaf == "to_q":
            up = up * (d ** -0.5 * math.log2(math.e))
    return down.to(torch.bfloat16), up.to(torch.bfloat16)


def merged_delta(adapters, path, scales):
    """sum_l scales[l] (alpha_l / r_l) B_l A_l of one module in fp64 - what a merge at those scales adds to the weight."""
    out = None
    for l, n in enumerate(adapters):
        if path not in adapters[n]:
            continue
        d, u, alpha = adapters[n][path]
        t = float(scales[l]) * (alpha / d.shape[0]) * (u.double() @ d.double())
        out = t if out is None else out + t
    return out


def _per_adapter(s, names, what):
    if isinstance(s, dict):
        bad = sorted(set(s) - set(names))
        if bad:
            raise ValueError(f"{what}: no regional adapter named {bad} is loaded (loaded: {names})")
        v = [float(s.get(n, 0.0)) for n in names]
    else:
        if len(names) != 1 and float(s) != 0.0:                         # (a plain 0 switches every adapter off, however many there are)
            raise ValueError(f"{what}: {len(names)} adapters are loaded ({names}), so a scale is a dict {{name: number}}, not a number")
        v = [float(s)] * len(names)
    if not all(math.isfinite(x) for x in v):
        raise ValueError(f"{what}: a scale must be finite, got {v}")
    return v + [0.0] * (MAX_ADAPTERS - len(v))


def slot_scales(names, n_regions, scale=0.0, regions=None, negative=None, base=None):
    """The scale matrix [prompt slot][MAX_ADAPTERS] in the engine's slot order [negative, region prompts ..., base]: `scale` is every slot's
    default, regions={i: s}, negative= and base= override it; a plain request has n_regions = 0 (slots [negative, base]).  s is a number
    when one adapter is loaded, else {name: number} (missing names: 0)."""
    regions = dict(regions or {})
    for i in regions:
        if not (isinstance(i, int) and 0 <= i < n_regions):
            raise ValueError(f"set_lora_scales: region {i!r} is outside this request's {n_regions} regions")
    every = _per_adapter(scale, names, "scale")
    rows = [_per_adapter(negative, names, "negative") if negative is not None else list(every)]
    for i in range(n_regions):
        rows.append(_per_adapter(regions[i], names, f"regions[{i}]") if i in regions else list(every))
    rows.append(_per_adapter(base, names, "base") if base is not None else list(every))
    return rows


def lora_request_from_specs(specs, who="--region_lora"):
    """['PATH[:TARGET[:SCALE]]', ...] -> (files, request): TARGET = all (every prompt slot, the default), base, negative or a region
    number, SCALE a finite number (default 1); files = {adapter name: path} - the name is the file's stem - and request = the keyword
    arguments of set_lora_scales.  Several specs may name the same file with different targets."""
    import os
    if isinstance(specs, str):
        specs = [specs]
    files, stems = {}, {}
    req = dict(scale={}, regions={}, negative={}, base={})
    for spec in specs:
        parts = str(spec).split(":")
        if not parts[0] or len(parts) > 3:
            raise ValueError(f"{who}: expected PATH[:TARGET[:SCALE]], got {spec!r}")
        path, target = parts[0], (parts[1] if len(parts) > 1 and parts[1] else "all")
        try:
            s = float(parts[2]) if len(parts) > 2 else 1.0
        except ValueError:
            raise ValueError(f"{who}: SCALE must be a number, got {parts[2]!r} in {spec!r}") from None
        if not math.isfinite(s):
            raise ValueError(f"{who}: SCALE must be finite, got {spec!r}")
        if path not in stems:
            stem = os.path.splitext(os.path.basename(path))[0]
            name, k = stem, 1
            while name in files:
                k += 1; name = f"{stem}_{k}"
            stems[path], files[name] = name, path
        name = stems[path]
        if target == "all":
            req["scale"][name] = s
        elif target in ("base", "negative"):
            req[target][name] = s
        elif target.isdigit():
            req["regions"].setdefault(int(target), {})[name] = s
        else:
            raise ValueError(f"{who}: TARGET must be all, base, negative or a region number, got {target!r} in {spec!r}")
    if len(files) > MAX_ADAPTERS:
        raise ValueError(f"{who}: {len(files)} adapters named; at most {MAX_ADAPTERS} can be resident")
    # a slot an adapter is not aimed at keeps the 'all' scale (or 0): the overrides carry the adapters' 'all' scales along
    for d in [req["negative"], req["base"]] + list(req["regions"].values()):
        for n, s in req["scale"].items():
            d.setdefault(n, s)
    return files, dict(scale=req["scale"], regions=req["regions"], negative=req["negative"] or None, base=req["base"] or None)


# ---------------------------------------------------------------------------------------------------------------- pipelines
def _read_checkpoint(src):
    if isinstance(src, dict):
        return src
    import os
    if not os.path.isfile(src):
        raise FileNotFoundError(f"regional LoRA: file not found: {src}")
    if str(src).endswith(".safetensors"):
        from safetensors.torch import load_file
        return load_file(src)
    return torch.load(src, map_location="cpu", weights_only=True)


def unet_shapes(config_dict):
    """module key -> an empty tensor of the weight's shape, from the engine's weight table (no device, no weights): what key resolution needs."""
    from .engine import Engine
    e = Engine(config_dict, 8, 8, device=-1)
    try:
        return {n: torch.empty(s, device="meta") for n, s in e.weight_table()}
    finally:
        e.close()


class RegionalLoraMixin:
    """`load_regional_loras({name: path_or_state_dict})` / `unload_regional_loras()` / `set_lora_scales(scale=, regions=, negative=)` /
    `clear_lora_scales()` of a pipeline (and of HipUNet2DConditionModel, which holds the engines): the adapters and the scale request are
    attributes, read by every sampling call right after it has set its text prompts (apply_lora_scales)."""
    regional_loras = None    # {name: modules} in load order, or None
    lora_request = None      # dict(scale=, regions=, negative=) or None

    def _rl_unet(self):
        return getattr(self, "unet", self)

    def load_regional_loras(self, named, attention_only=False, targets="attention"):
        """named: {name: path or state dict}, 1 .. 4 adapters whose padded ranks add up to at most 128.  Engines are built with the adapters
        from now on (existing ones are rebuilt on their next use); every scale starts at 0.  On a rank whose UNet weights arrive by
        broadcast, load BEFORE the first engine exists.  targets="transformer" also takes adapters on ff.net.0.proj, ff.net.2, proj_in and
        proj_out; the engines carry those modules only when some loaded adapter has a tensor there, so a file of attention tensors runs
        the same path and bits under either value.  Returns {name: report} (applied / dropped / text_encoder / alpha_default)."""
        check_targets(targets)
        u = self._rl_unet()
        if not isinstance(named, dict) or not named:
            raise ValueError("load_regional_loras: a dict {name: path or state dict} with at least one adapter")
        shapes = u._state_dict if isinstance(u._state_dict, dict) else unet_shapes(u.config_dict)
        adapters, reports = {}, {}
        for name, src in named.items():
            adapters[str(name)], reports[str(name)] = parse_adapter(shapes, _read_checkpoint(src), attention_only, targets)
        rank_layout(adapters)                                         # more than 4 adapters / 128 rank columns: a ValueError naming the numbers
        u.install_regional_loras(adapters)
        self.regional_loras, self.lora_request = adapters, None
        return reports

    def unload_regional_loras(self):
        self._rl_unet().install_regional_loras(None)
        self.regional_loras = self.lora_request = None

    def set_lora_scales(self, scale=0.0, regions=None, negative=None, base=None):
        """`scale`: the default of every prompt slot (the negative prompt included); `negative=` overrides it for the negative prompt,
        `regions={i: s}` for rich-text region i, `base=` for the base prompt.  s is a number when one adapter is loaded, else {name: number} (missing names: 0)."""
        if not self.regional_loras:
            raise ValueError(f"{type(self).__name__}.set_lora_scales: no regional adapter loaded (load_regional_loras first)")
        if regions is not None and not isinstance(regions, dict):
            raise ValueError(f"set_lora_scales: regions must be a dict {{region index: scale}}, got {type(regions).__name__}")
        names = list(self.regional_loras)
        slot_scales(names, max([k + 1 for k in (regions or {}) if isinstance(k, int) and k >= 0] or [0]), scale, regions, negative, base)      # names, types and finiteness, now
        self.lora_request = dict(scale=scale, regions=dict(regions or {}), negative=negative, base=base)

    def clear_lora_scales(self):
        self.lora_request = None

    def lora_slot_scales(self, n_prompts, rich):
        """The scale matrix of a call that sets n_prompts prompts - [negative, base] or [negative, region prompts ..., base] -, or None
        without a request.  A region index beyond the request's regions is a ValueError - raised here, before anything is launched."""
        r = self.lora_request
        if r is None or not self.regional_loras:
            return None
        # (a plain pass - [negative, base] - has no regions: regions= is the rich pass's alone, as with set_control)
        return slot_scales(list(self.regional_loras), n_prompts - 2, r["scale"], r["regions"] if rich else None, r["negative"], r.get("base"))

    def apply_lora_scales(self, eng, scales):
        """Right after eng.set_prompts (which reset every scale)."""
        if scales is not None and any(v != 0.0 for row in scales for v in row):
            eng.set_lora_scales(scales)
