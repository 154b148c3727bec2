"""Oracle side of the weight-influence tests (tests/test_weight_influence_ref.py: CPU; tests/test_weight_influence_gpu.py: engine).

For every 1-D tensor k of a UNet state dict (biases, norm scales and offsets) the ORACLE ALONE chooses a perturbation that moves the
output of the module that owns k by a known, large amount; the GPU test then asks the engine for the same change.

  owner(k)         the traceable module (OracleUNet ctl["trace"] / rt_unet_forward_trace) whose name prefixes k; conv_norm_out.* and
                   conv_out.bias are observed at conv_out, time_embedding.* and add_embedding.* at down_blocks.0.resnets.0 (the first
                   consumer of the embedding), conv_in.bias at conv_in
  perturbation     sd_k = sd with k := k + A u, u ~ U(-1, 1) drawn by a torch CPU generator seeded with the tensor's index in the state
                   dict's key order; A walks LADDER and stops at the first A with rho >= RHO_STOP, else keeps the largest
  rho_k            rel-L2 of the oracle's change at the owner's output: |trace_k - trace_0| / |trace_0|
  prompt scale     transformer_blocks.*.norm2.* only: the prompt embeddings times NORM2_EMB_SCALE.  norm2 feeds nothing but attn2's
                   to_q; with unit-variance embeddings and 1 / sqrt(fan_in) weights the attn2 branch is tiny next to the residual trunk
                   and rho stays at 1e-4; scaled keys make the softmax sharp and the values large

Condition (checked on the CPU, not measured on the GPU): every tensor reaches rho >= RHO_MIN.  With LADDER = (0.5, 2), the scale 6 and
the inputs of `inputs()`, 355 of the 356 1-D tensors of TINY_XL_CONFIG (latent 16x16) and 403 of the 404 of TINY_SD_CONFIG (latent 16x32,
the smallest grid its four levels run: 2x4 = 8 tokens at the deepest attention) meet it.  The two that fall short -
time_embedding.linear_1.bias (XL: rho 0.096 at A = 2) and down_blocks.0.attentions.1.transformer_blocks.0.norm1.weight (SD: 0.063) - set
the rule for their classes: `time_embedding.*` and `transformer_blocks.*.norm1.weight` walk one more rung, A = 4 (`ladder()`), decided
from the oracle's figures alone.  Neither class can overflow the fp16 trunk: the time embedding is fp32 until the resnets add it, and a
norm1 scale in [-3, 5] scales attn1's inputs, whose output stays a convex combination of the value rows.  Everything else stays at A <= 2.

Resolution: the bound is 0.115 at rho = 0.3 and 0.315 at rho = 0.1, so an error of a few tens of percent in ONE tensor's influence
passes.  What fails is a tensor that is dropped, applied twice, applied with the wrong sign or swapped with a same-shaped sibling: each
gives rel_l2(D_eng, D_ref) >= 1.
"""
import contextlib

import torch

from oracle.unet import OracleUNet

LADDER = (0.5, 2.0)
RHO_STOP, RHO_MIN = 0.3, 0.1
NORM2_EMB_SCALE = 6.0
FORWARD_BOUND = 1.5e-2          # the project's forward bound (tests/test_engine_gpu.py), per module in tests/test_unet_trace_gpu.py
T = 701.0
THREADS = 16


@contextlib.contextmanager
def oracle_threads(n=THREADS):
    """The fp32 oracle on a pool of 16 threads (the machines these tests run on show many more CPUs than a job may use)."""
    old = torch.get_num_threads()
    torch.set_num_threads(n)
    try:
        yield
    finally:
        torch.set_num_threads(old)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


def bound(rho, eps=FORWARD_BOUND):
    """Bound on rel_l2(D_eng, D_ref) for D = trace(perturbed) - trace(base), from the per-module bound eps on each trace by the triangle
    inequality: |D_eng - D_ref| <= eps |t_k| + eps |t_0| <= eps (2 + rho) |t_0| and |D_ref| = rho |t_0|."""
    return eps * (2.0 + rho) / rho


def trace_modules(cfg):
    """Names of the traceable modules in execution order, from the config alone (the oracle's ctl["trace"] keys and the engine's
    rt_trace_module_info list are pinned against it in tests/test_weight_influence_ref.py)."""
    boc = cfg["block_out_channels"]
    n = len(boc)
    lpb = cfg["layers_per_block"]
    lpb = (lpb,) * n if isinstance(lpb, int) else tuple(lpb)
    out = ["conv_in"]
    for i, bt in enumerate(cfg["down_block_types"]):
        for j in range(lpb[i]):
            out.append(f"down_blocks.{i}.resnets.{j}")
            if bt == "CrossAttnDownBlock2D":
                out.append(f"down_blocks.{i}.attentions.{j}")
        if i != n - 1:
            out.append(f"down_blocks.{i}.downsamplers.0.conv")
    out += ["mid_block.resnets.0", "mid_block.attentions.0", "mid_block.resnets.1"]
    for i, bt in enumerate(cfg["up_block_types"]):
        for j in range(lpb[n - 1 - i] + 1):
            out.append(f"up_blocks.{i}.resnets.{j}")
            if bt == "CrossAttnUpBlock2D":
                out.append(f"up_blocks.{i}.attentions.{j}")
        if i != n - 1:
            out.append(f"up_blocks.{i}.upsamplers.0.conv")
    out.append("conv_out")
    return out


def owner(name, modules):
    if name.startswith(("conv_norm_out.", "conv_out.")):
        return "conv_out"
    if name.startswith(("time_embedding.", "add_embedding.")):
        return "down_blocks.0.resnets.0"
    hits = [m for m in modules if name.startswith(m + ".")]
    assert len(hits) == 1, (name, hits)
    return hits[0]


def ladder(name):
    """The amplitudes a tensor walks (module docstring: two classes take a third rung)."""
    if name.startswith("time_embedding.") or (".transformer_blocks." in name and name.endswith(".norm1.weight")):
        return LADDER + (4.0,)
    return LADDER


def group_of(name):
    """The parametrisation of the tests: the top-level block of a tensor and, inside the blocks, the kind of its module (resnets /
    attentions / downsamplers / upsamplers) - the oracle's time for a case stays near 10 s."""
    if name.startswith(("conv_in.", "time_embedding.", "add_embedding.")):
        return "stem"
    if name.startswith(("conv_norm_out.", "conv_out.")):
        return "out"
    parts = name.split(".")
    return ".".join(parts[:2] if parts[0] == "mid_block" else parts[:3])


def groups(cfg):
    """Every group that owns a tensor, in execution order."""
    out = ["stem"]
    for m in trace_modules(cfg)[1:-1]:
        g = group_of(m + ".bias")
        if g not in out:
            out.append(g)
    return out + ["out"]


def one_d_tensors(sd):
    """[(index in the state dict's key order, name)] of every 1-D tensor."""
    return [(i, k) for i, k in enumerate(sd) if sd[k].dim() == 1]


def needs_scaled_prompt(name):
    return ".transformer_blocks." in name and ".norm2." in name


def inputs(cfg, h, w, seed=7):
    """One stream: latent, prompt embeddings [1, 77, D], and SDXL's pooled embedding / time ids."""
    g = torch.Generator().manual_seed(seed)
    xl = cfg.get("addition_embed_type") == "text_time"
    emb = torch.randn(1, 77, cfg["cross_attention_dim"], generator=g)
    lat = torch.randn(1, 4, h, w, generator=g)
    pooled = tid = None
    if xl:
        pooled = torch.randn(1, cfg["projection_class_embeddings_input_dim"] - 6 * cfg["addition_time_embed_dim"], generator=g)
        tid = torch.tensor([[h * 8.0, w * 8.0, 0.0, 0.0, h * 8.0, w * 8.0]])
    return dict(lat=lat, emb=emb, pooled=pooled, tid=tid, xl=xl)


def direction(sd, index, name):
    g = torch.Generator().manual_seed(index)
    return torch.rand(sd[name].shape, generator=g) * 2 - 1


# The LayerNorm fold (csrc/gemm16.hip "LNF": norm1/2/3 baked into W' = gamma W and c = b + W beta) runs at SDXL's widths only, which the
# tiny configs never reach.  The smallest slice that takes it: two levels (640, 1280) with SDXL's head dim 64, one resnet and one
# transformer layer per level.  The latent is the smallest at which every consumer of the block's LayerNorms has the folded form - the
# 16x16x32 family takes a projection from 256 tokens per stream on, and attn1's V^T product stays unsplit (split-K has no fold) from
# 4 cdiv(C, 128) cdiv(tokens, 128) > 96 on: more than 256 tokens at 1280 channels, so 40x32 -> 1280 / 320 tokens.  The GPU test does
# not trust this arithmetic: it asks rt_op_ln_gemm for every consumer shape and asserts that none answers "no folded form".
FOLD_CONFIG = dict(
    in_channels=4, out_channels=4, block_out_channels=(640, 1280),
    down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D"), up_block_types=("CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
    layers_per_block=1, transformer_layers_per_block=(1, 1), attention_head_dim=(10, 20), cross_attention_dim=64,
    norm_num_groups=32, norm_eps=1e-5, use_linear_projection=True, addition_embed_type=None, addition_time_embed_dim=None,
    projection_class_embeddings_input_dim=None)
FOLD_LATENT = (40, 32)
FOLD_OWNERS = ("down_blocks.0.attentions.0", "down_blocks.1.attentions.0")      # one transformer block per level


def fold_tensors(sd):
    """[(index, name)]: norm1/2/3.*, attn*.to_out.0.bias, ff.net.*.bias and proj_in / proj_out.bias of FOLD_OWNERS."""
    keep = (".norm1.", ".norm2.", ".norm3.", ".to_out.0.bias", ".ff.net.0.proj.bias", ".ff.net.2.bias", ".proj_in.bias", ".proj_out.bias")
    return [(i, k) for i, k in one_d_tensors(sd) if k.startswith(tuple(o + "." for o in FOLD_OWNERS)) and any(t in k for t in keep)]


class Influence:
    """Oracle forwards of one (config, weights, inputs): the base traces (prompt scale 1 and NORM2_EMB_SCALE, one full forward each, computed
    on first use) and, per tensor, the chosen perturbation with the oracle's change at the owner."""

    def __init__(self, cfg, sd, inp, stop=None):
        """stop: the last module any tensor of interest is observed at (the base forwards end there too); None = the whole UNet."""
        self.cfg, self.sd, self.inp, self.stop = cfg, sd, inp, stop
        self.oracle = OracleUNet(cfg, sd)
        self.modules = trace_modules(cfg)
        self._base = {}

    def _forward(self, scale, ctl):
        i = self.inp
        added = {"text_embeds": i["pooled"], "time_ids": i["tid"]} if i["xl"] else None
        with torch.no_grad(), oracle_threads():
            return self.oracle.forward(i["lat"], T, i["emb"] * scale, added, ctl=ctl)

    def base(self, scale):
        if scale not in self._base:
            tr = {}
            self._forward(scale, {"trace": tr, "trace_stop": self.stop})
            self._base[scale] = tr
        return self._base[scale]

    def perturbed_trace(self, name, value, own, scale):
        old = self.oracle.sd[name]
        self.oracle.sd[name] = value.float()
        try:
            return self._forward(scale, {"trace_stop": own})
        finally:
            self.oracle.sd[name] = old

    def choose(self, index, name):
        """-> dict(name, owner, A, scale, rho, value (the perturbed tensor), d_ref (the oracle's change at the owner))"""
        own = owner(name, self.modules)
        scale = NORM2_EMB_SCALE if needs_scaled_prompt(name) else 1.0
        t0 = self.base(scale)[own]
        u = direction(self.sd, index, name)
        for A in ladder(name):
            value = self.sd[name].float() + A * u
            d = self.perturbed_trace(name, value, own, scale) - t0
            rho = (d.double().pow(2).sum() / t0.double().pow(2).sum()).sqrt().item()
            if rho >= RHO_STOP:
                break
        return dict(name=name, owner=own, A=A, scale=scale, rho=rho, value=value, d_ref=d)
