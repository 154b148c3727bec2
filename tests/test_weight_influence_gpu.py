"""Every bias, norm scale and norm offset of the UNet reaches the launch it belongs to - tensor by tensor, through the engine's own
wiring (state dict -> rt_bind_weight -> packed arena / folded W', c / temb_all table -> launch arguments), not through hand-made kernel
arguments.

The final eps cannot see most 1-D tensors: set one at a time to its neutral value and about 80 % of them move the final output by less
than the forward bound 1.5e-2.  So the change is observed where it is not yet damped: at the output of the module that owns the tensor
(rt_unet_forward_trace), with a perturbation the ORACLE chose so that its own change there is rho >= 0.1 (tests/weight_influence_ref.py
holds the rules; tests/test_weight_influence_ref.py checks on the CPU that every tensor meets the condition).

Per tensor k, two engine forwards with trace (base, and k re-bound to its perturbed value) and two oracle forwards;
D = trace(perturbed) - trace(base):

    rel_l2(D_eng, D_ref) <= 1.5e-2 (2 + rho_k) / rho_k        (0.115 at rho = 0.3, 0.315 at rho = 0.1)

which follows from the per-module bound of tests/test_unet_trace_gpu.py by the triangle inequality (no module has a bound of its own).
A dropped tensor, one applied twice, one applied with the wrong sign and one swapped with a same-shaped sibling all give >= 1.0; an
error of a few tens of percent in one tensor's influence is NOT resolved.  Once per group the comparison is shown to fail for D_eng = 0
and D_eng = 2 D_ref.

Re-binding goes the way LoRA goes (Engine.bind_weight of the one tensor on a live engine), so the test also pins what a re-bind refreshes:
the packed vectors at once, the folded (W', c) at the next forward, the time_emb_proj table by construction (read from the arena every
forward).  What rt_set_prompts derived cannot follow - the addition embeddings of add_embedding.* - and the engine says so: a forward
behind such a re-bind is an error until the prompts are set again (asserted here).  After a group its tensors are back and the base
trace is bit for bit what it was.

Measured on the MI355X (all tensors inside their bound, no tensor's influence was wrong in the engine):
  config    tensors  smallest rho  largest rel_l2(D_eng, D_ref)  its bound  the tensor
  tiny XL   356      0.164         0.0694                        0.102      up_blocks.0.attentions.2.transformer_blocks.0.norm2.weight
  tiny SD   404      0.131         0.0506                        0.054      up_blocks.1.attentions.2.transformer_blocks.0.norm2.weight
  fold      24       0.186         0.0165 (fold off: 0.0161)     0.050      down_blocks.1.attentions.0.transformer_blocks.0.norm2.weight
Closest to its bound: tiny XL up_blocks.0.attentions.1.transformer_blocks.0.norm2.weight, 0.0553 of 0.056.  The norm2 pairs are the
loudest rows throughout (0.01 - 0.07; everything else stays below 0.026, the biases of the sampler convolutions at 5e-4): their prompt
embeddings are scaled by 6 and norm2.weight by up to 3, so attn2's logits are up to 18 times their usual size and the bf16 rounding of
Q and K moves a sharp softmax - rounding of that regime, not wiring.  The engine is deterministic, so the margin does not wander.

The LayerNorm fold (norm1/2/3 baked into W' = gamma W, c = b + W beta) only runs at SDXL's widths: one more case on a two-level
(640, 1280) slice at the smallest latent whose transformer blocks take it (asserted through rt_op_ln_gemm, which answers -5 for a shape
without a folded form), once folded and once with the fold switched off (rt_op_gemm_debug bit 22); both meet the same bound against the
oracle.  Oracle time for that case: about 25 s (0.3 - 0.6 s per forward that ends at the observed transformer).
"""
import ctypes as C
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict  # noqa: E402
import weight_influence_ref as W  # noqa: E402

DEV = "cuda:0"
CASES = {"tiny_xl": (TINY_XL_CONFIG, 16, 16), "tiny_sd": (TINY_SD_CONFIG, 16, 32), "fold": (W.FOLD_CONFIG,) + W.FOLD_LATENT}
PARAMS = [(which, g) for which in ("tiny_xl", "tiny_sd") for g in W.groups(CASES[which][0])]


class Rig:
    """One engine and one oracle on the same weights and inputs; the base traces of both are computed once per (module, prompt scale)."""

    def __init__(self, which):
        from rich_text_to_image_amd.engine import Engine
        cfg, h, w = CASES[which]
        self.which, self.cfg, self.h, self.w = which, cfg, h, w
        self.sd = random_state_dict(cfg, seed=11)
        self.inp = W.inputs(cfg, h, w)
        self.inf = W.Influence(cfg, self.sd, self.inp, stop=W.FOLD_OWNERS[-1] if which == "fold" else None)
        self.eng = Engine(cfg, h, w, device=0, max_streams=1, max_prompts=1)
        self.eng.load_state_dict(self.sd)
        self.x = self.inp["lat"].to(DEV)
        self.scale = None
        self.base = {}
        self.choice = {}

    def prompts(self, scale, force=False):
        if scale != self.scale or force:
            i = self.inp
            if i["xl"]:
                self.eng.set_prompts((i["emb"] * scale).to(DEV), i["pooled"].to(DEV), i["tid"])
            else:
                self.eng.set_prompts((i["emb"] * scale).to(DEV))
            self.eng.set_fontsize(None, None)
            self.scale = scale

    def trace(self, module, scale):
        self.prompts(scale)
        return self.eng.unet_forward(self.x, W.T, [0], trace=module)[1].cpu()

    def base_trace(self, module, scale, tag=""):
        key = (module, scale, tag)
        if key not in self.base:
            self.base[key] = self.trace(module, scale)
        return self.base[key]

    def bind(self, name, value):
        t = value.to(DEV)
        self.eng.bind_weight(name, t)
        self.eng.synchronize()               # the pack launch reads t on the engine's stream

    def chosen(self, index, name):
        if name not in self.choice:
            self.choice[name] = self.inf.choose(index, name)
        return self.choice[name]


_rigs = {}


@pytest.fixture(scope="module")
def rigs():
    def get(which):
        if which not in _rigs:
            _rigs[which] = Rig(which)
        return _rigs[which]
    yield get
    for r in _rigs.values():
        r.eng.close()
    _rigs.clear()


def within(d_eng, d_ref, rho):
    """(measured, bound, measured <= bound) of the comparison every tensor is held to."""
    m, b = W.rel_l2(d_eng, d_ref), W.bound(rho)
    return m, b, m <= b


def run_group(rig, tensors, tag=""):
    """The comparison for every (index, name) of `tensors`; prints one row per tensor and returns the rows that miss their bound."""
    from rich_text_to_image_amd.engine import RtError
    rows, last = [], None
    for i, k in tensors:
        c = rig.chosen(i, k)
        assert c["rho"] >= W.RHO_MIN, (k, c["rho"])                         # the oracle's condition (CPU: tests/test_weight_influence_ref.py)
        t0 = rig.base_trace(c["owner"], c["scale"], tag)
        derived_from_prompts = k.startswith("add_embedding.")
        rig.bind(k, c["value"])
        try:
            if derived_from_prompts:                                       # the addition embeddings rt_set_prompts cached are stale now
                with pytest.raises(RtError, match="rt_set_prompts"):
                    rig.eng.unet_forward(rig.x, W.T, [0])
                rig.prompts(c["scale"], force=True)
            tk = rig.trace(c["owner"], c["scale"])
        finally:
            rig.bind(k, rig.sd[k])
            if derived_from_prompts:
                rig.prompts(c["scale"], force=True)
        m, b, ok = within(tk - t0, c["d_ref"], c["rho"])
        print(f"{rig.which}{tag} {k:<75s} @ {c['owner']:<28s} A {c['A']:.1f} rho {c['rho']:.3f} bound {b:.3f} measured {m:.4f}{'' if ok else '   MISSES'}")
        rows.append((k, c["rho"], b, m, ok))
        last = c
    # positive control: the same comparison refuses a tensor that has no effect and one that is applied twice
    for fake in (torch.zeros_like(last["d_ref"]), 2 * last["d_ref"]):
        assert not within(fake, last["d_ref"], last["rho"])[2]
    # every tensor is back: the base trace is what it was, bit for bit
    assert torch.equal(rig.trace(last["owner"], last["scale"]), rig.base_trace(last["owner"], last["scale"], tag)), "re-binding the original tensors did not restore the engine"
    worst = max(rows, key=lambda r: r[3] / r[2])
    print(f"{rig.which}{tag}: {len(rows)} tensors, smallest rho {min(r[1] for r in rows):.3f}, largest measured {max(r[3] for r in rows):.4f}, "
          f"closest to its bound {worst[0]} ({worst[3]:.4f} of {worst[2]:.3f})")
    return [r for r in rows if not r[4]]


@pytest.mark.parametrize("which,group", PARAMS, ids=[f"{a}-{b}" for a, b in PARAMS])
def test_every_one_d_tensor_has_the_oracles_influence(which, group, rigs):
    rig = rigs(which)
    tensors = [(i, k) for i, k in W.one_d_tensors(rig.sd) if W.group_of(k) == group]
    assert tensors
    missed = run_group(rig, tensors)
    assert not missed, missed


def test_rebinding_a_weight_that_set_prompts_reads_discards_the_prompts(rigs):
    """attn2.to_k / to_v feed the K / V^T caches rt_set_prompts builds: after a re-bind (here of the SAME values) the engine refuses
    forwards until the prompts are set again, and is then bit for bit where it was.  A weight no cache depends on needs nothing."""
    from rich_text_to_image_amd.engine import RtError
    rig = rigs("tiny_xl")
    rig.prompts(1.0, force=True)
    before = rig.eng.unet_forward(rig.x, W.T, [0])
    rig.bind("mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight", rig.sd["mid_block.attentions.0.transformer_blocks.0.attn1.to_q.weight"])
    assert torch.equal(rig.eng.unet_forward(rig.x, W.T, [0]), before)
    for k in ("mid_block.attentions.0.transformer_blocks.1.attn2.to_k.weight", "down_blocks.1.attentions.0.transformer_blocks.0.attn2.to_v.weight"):
        rig.bind(k, rig.sd[k])
        with pytest.raises(RtError, match="rt_set_prompts"):
            rig.eng.unet_forward(rig.x, W.T, [0])
        rig.prompts(1.0, force=True)
        assert torch.equal(rig.eng.unet_forward(rig.x, W.T, [0]), before)


def _fold_taken(lib, tokens, Cw):
    """rt_op_ln_gemm for the four consumer shapes of a transformer block of width Cw at `tokens` tokens per stream (stacked to_q | to_k,
    V^T, attn2.to_q, GEGLU): 0 = folded form, -5 = none."""
    from rich_text_to_image_amd.engine import _ptr
    g = torch.Generator().manual_seed(1)
    x = torch.randn(tokens, Cw, generator=g).to(DEV).to(torch.float16)
    gamma, beta = torch.ones(Cw, device=DEV), torch.zeros(Cw, device=DEV)
    rcs = {}
    for label, N, epi, vt in (("to_q|to_k", 2 * Cw, 0, 0), ("to_v^T", Cw, 0, 1), ("attn2.to_q", Cw, 0, 0), ("ff.net.0 GEGLU", 8 * Cw, 3, 0)):
        Wt = (torch.randn(N, Cw, generator=g) * Cw ** -0.5).to(DEV).to(torch.bfloat16)
        out = torch.empty(Cw if vt else tokens, tokens if vt else (N // 2 if epi == 3 else N), device=DEV, dtype=torch.bfloat16)
        rcs[label] = lib.rt_op_ln_gemm(_ptr(x), _ptr(gamma), _ptr(beta), _ptr(Wt), None, _ptr(out), tokens, N, Cw, epi, vt, tokens, None, None, 320, None)
        torch.cuda.synchronize()
    return rcs


@pytest.mark.parametrize("fold", ["folded", "fold_off"])
def test_layernorm_fold_width_tensors_have_the_oracles_influence(fold, rigs):
    rig = rigs("fold")
    lib = rig.eng.lib
    h, w = W.FOLD_LATENT
    boc = W.FOLD_CONFIG["block_out_channels"]
    for lvl, Cw in enumerate(boc):                                         # the route query: every consumer of both levels has the folded form
        rcs = _fold_taken(lib, (h >> lvl) * (w >> lvl), Cw)
        assert all(rc == 0 for rc in rcs.values()), (Cw, rcs)
    tensors = W.fold_tensors(rig.sd)
    assert len(tensors) == 24
    base_flags = int(os.environ.get("RTDIFF_DEBUG_FLAGS", "0"))
    assert not base_flags & (1 << 22)
    own = W.FOLD_OWNERS[-1]
    folded = rig.base_trace(own, 1.0, "")
    if fold == "folded":
        missed = run_group(rig, tensors)
    else:
        lib.rt_op_gemm_debug(base_flags | (1 << 22))
        try:
            unfolded = rig.base_trace(own, 1.0, " fold off")
            missed = run_group(rig, tensors, " fold off")
        finally:
            lib.rt_op_gemm_debug(base_flags)
        # the switch did switch: LayerNorm launches round the normalised rows to bf16, the fold rounds the trunk - different bits
        assert not torch.equal(unfolded, folded)
        assert W.rel_l2(unfolded, folded) < 2 * W.FORWARD_BOUND
    assert not missed, missed
