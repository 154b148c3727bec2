"""ControlNet references (test infrastructure): the CPU restatement of diffusers' ControlNetModel forward and of the UNet forward with its
residuals, as a companion of oracle.unet.OracleUNet; the fp64 restatements of the residual add (csrc/control.hip) and of the hint embedder;
the bars of both, derived here from where the kernels round; synthetic checkpoints.

The formulas and key names are diffusers' ControlNetModel / ControlNetConditioningEmbedding as remembered ([memory]): diffusers is not
installed where these tests run, so parity with it is unpinned, like the rest of that row of the oracle.

  ControlNetModel.forward(sample, t, ctx, controlnet_cond, conditioning_scale):
      emb     = time_embedding(t) (+ add_embedding(text_embeds | time_ids))
      x       = conv_in(sample) + controlnet_cond_embedding(controlnet_cond)
      skips   = [x] + every down resnet (/ attention) output + every down-sampler output              (the UNet's own encoder, own weights)
      mid     = mid_block(x)
      down_k  = conditioning_scale * controlnet_down_blocks[k](skips[k]),   mid_r = conditioning_scale * controlnet_mid_block(mid)
  UNet2DConditionModel.forward(..., down_block_additional_residuals, mid_block_additional_residual):
      skips[k] += down_k for every k behind the down path - which has run on the UN-added tensors -, sample += mid_r behind the mid block.
  ControlNetConditioningEmbedding: conv_in, SiLU, then blocks[0..5] each followed by SiLU (blocks[2 i]: ch[i] -> ch[i], stride 1;
      blocks[2 i + 1]: ch[i] -> ch[i + 1], stride 2; all 3x3, pad 1), then conv_out (ch[3] -> block_out_channels[0]) without activation.
"""
import math

import torch
import torch.nn.functional as F

from oracle.shapes import weight_shapes
from oracle.unet import OracleUNet, timestep_embedding

P = "controlnet."
CE = "controlnet_cond_embedding."
TINY_EMBED = (16, 32, 32, 64)           # the embedder of the tiny configs (multiples of 8, as rt_config asks)

# ---------------------------------------------------------------------------------------------------------------- synthetic checkpoints
# Weight scales, chosen on the CPU references alone so that the discrimination checks of tests/test_controlnet.py hold with their factors
# (a dropped residual, a dropped embedder bias ... cannot pass a bar):
ZERO_CONV_GAIN = 1.0                     # zero convolutions N(0, 1 / fan_in): already 0.7 - 1.1 from the uncontrolled oracle on the forward cases (10 x bar = 0.15)
EMBED_BIAS_STD = 0.5                     # embedder biases N(0, 0.5^2): a dropped bias moves the embedding far beyond its bar


def _embed_shapes(c0, ch, hint_channels):
    s = {CE + "conv_in": (ch[0], hint_channels)}
    for i in range(3):
        s[CE + f"blocks.{2 * i}"] = (ch[i], ch[i])
        s[CE + f"blocks.{2 * i + 1}"] = (ch[i + 1], ch[i])
    s[CE + "conv_out"] = (c0, ch[3])
    return s


def skip_channels(cfg):
    """Channels of the UNet's skips in push order: conv_in, every down resnet (/ attention), every down-sampler."""
    boc = cfg["block_out_channels"]
    n = len(boc)
    lpb = cfg["layers_per_block"] if isinstance(cfg["layers_per_block"], (tuple, list)) else (cfg["layers_per_block"],) * n
    out = [boc[0]]
    for i in range(n):
        out += [boc[i]] * lpb[i]
        if i != n - 1:
            out.append(boc[i])
    return out


def skip_sources(cfg):
    """The module whose output is skip k (the names of oracle.unet's trace), in push order."""
    n = len(cfg["block_out_channels"])
    lpb = cfg["layers_per_block"] if isinstance(cfg["layers_per_block"], (tuple, list)) else (cfg["layers_per_block"],) * n
    out = ["conv_in"]
    for i, bt in enumerate(cfg["down_block_types"]):
        kind = "attentions" if bt == "CrossAttnDownBlock2D" else "resnets"
        out += [f"down_blocks.{i}.{kind}.{j}" for j in range(lpb[i])]
        if i != n - 1:
            out.append(f"down_blocks.{i}.downsamplers.0.conv")
    return out


def control_state_dict(cfg, seed=0, embed_channels=TINY_EMBED, hint_channels=3, zero_gain=ZERO_CONV_GAIN):
    """A synthetic ControlNet for UNet config `cfg` in diffusers' ControlNetModel layout (keys WITHOUT the engine's "controlnet." prefix):
    the encoder as oracle.unet.random_state_dict draws it, the embedder with visible biases, the zero convolutions N(0, gain^2 / fan_in) -
    not zero: a trained ControlNet's are not, and zeros would test nothing."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name, shape in weight_shapes(cfg).items():
        if not name.startswith(("conv_in.", "time_embedding.", "add_embedding.", "down_blocks.", "mid_block.")):
            continue
        if name.endswith(".weight") and len(shape) >= 2:
            fan_in = math.prod(shape[1:])
            sd[name] = (torch.rand(shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
        elif name.endswith(".weight"):
            sd[name] = 1.0 + 0.1 * (torch.rand(shape, generator=g) * 2 - 1)
        else:
            sd[name] = 0.05 * (torch.rand(shape, generator=g) * 2 - 1)
    for name, (co, ci) in _embed_shapes(cfg["block_out_channels"][0], embed_channels, hint_channels).items():
        sd[name + ".weight"] = torch.randn(co, ci, 3, 3, generator=g) * (1.5 / math.sqrt(9 * ci))
        sd[name + ".bias"] = torch.randn(co, generator=g) * EMBED_BIAS_STD
    for k, c in enumerate(skip_channels(cfg)):
        sd[f"controlnet_down_blocks.{k}.weight"] = torch.randn(c, c, 1, 1, generator=g) * (zero_gain / math.sqrt(c))
        sd[f"controlnet_down_blocks.{k}.bias"] = torch.randn(c, generator=g) * 0.05
    c = cfg["block_out_channels"][-1]
    sd["controlnet_mid_block.weight"] = torch.randn(c, c, 1, 1, generator=g) * (zero_gain / math.sqrt(c))
    sd["controlnet_mid_block.bias"] = torch.randn(c, generator=g) * 0.05
    return sd


def zeroed(cn_sd):
    """The same ControlNet with zero-valued zero convolutions (what an untrained one holds)."""
    return {k: (torch.zeros_like(v) if k.startswith(("controlnet_down_blocks.", "controlnet_mid_block.")) else v) for k, v in cn_sd.items()}


def prefixed(cn_sd):
    return {P + k: v for k, v in cn_sd.items()}


def make_hint(h, w, seed=5, channels=3):
    """A hint image [channels, 8 h, 8 w] in 0 .. 1 on the k / 255 grid: smooth blobs with hard edges, like an edge or depth map."""
    g = torch.Generator().manual_seed(seed)
    low = torch.rand(1, channels, max(2, h // 2), max(2, w // 2), generator=g)
    img = F.interpolate(low, size=(8 * h, 8 * w), mode="bilinear", align_corners=False)[0]
    img = torch.where(img > 0.55, torch.ones_like(img), img * 0.6)
    return (img * 255).round() / 255


# ---------------------------------------------------------------------------------------------------------------- the hint embedder
EMBED_LAYERS = ("conv_in", "blocks.0", "blocks.1", "blocks.2", "blocks.3", "blocks.4", "blocks.5", "conv_out")


def _bf16(t):
    return t.float().to(torch.bfloat16).double()


def embed_ref(cn_sd, hint, *, emulate=False, no_silu_after=None, stride_all=None, pad=1, drop_bias=None):
    """controlnet_cond_embedding on hint [Ch, H, W] -> [C0, H / 8, W / 8], fp64.

    emulate=False: the exact restatement - fp64 arithmetic on the checkpoint's own (fp32) weights, nothing rounded.
    emulate=True:  rounds where an honest kernel does: the hint and every weight to bf16 (the operands of the MFMA), exact products
                   and sums (fp64 stands in for the fp32 accumulator, whose own error, <= K 2^-24 relative to the sum of magnitudes
                   with K <= 9 x 64 taps, is two orders below one bf16 rounding), the fp32 bias, SiLU on that value, and ONE rounding to
                   bf16 of every activation that the next convolution reads; conv_out's result is not rounded (it leaves as fp32).
    The keyword faults are for the discrimination checks: a missing SiLU behind layer `no_silu_after`, every stride-2 layer run with
    `stride_all`, another `pad`, the bias of layer `drop_bias` dropped."""
    x = hint.double()[None]
    if emulate:
        x = _bf16(x)
    for name in EMBED_LAYERS:
        w, b = cn_sd[CE + name + ".weight"].double(), cn_sd[CE + name + ".bias"].double()
        if emulate:
            w = _bf16(w)
        stride = 2 if name in ("blocks.1", "blocks.3", "blocks.5") else 1
        if stride_all is not None and stride == 2:
            stride = stride_all
        x = F.conv2d(x, w, None if drop_bias == name else b, stride=stride, padding=pad)
        if name != "conv_out":
            if no_silu_after != name:
                x = F.silu(x)
            if emulate:
                x = _bf16(x)
    return x[0]


# The bar of the embedder, on rel-L2 against the exact restatement:  EMBED_MARGIN x rel_l2(emulation, exact).
# (It is the bar of a kernel with bf16 operands and fp32 accumulation per layer.  The engine's embedder has since moved to fp32 arithmetic
# and sits orders of magnitude inside it; the bar is kept as derived - it is what an implementation on the MFMA routes would have to meet.)
# The emulation IS an honest kernel's error up to three things it does not model, each bounded by what it does model:
#   - the fp32 accumulation order and the fast exponential of SiLU: <= 2^-21 relative per layer, against 2^-9 per bf16 rounding;
#   - rounding flips: where fp32 and fp64 accumulators straddle a bf16 rounding boundary the kernel's activation differs from the
#     emulation's by one bf16 ulp - at most ONE more rounding error of the size already counted, on a small share of the elements;
#   - correlation: the flips and the emulation's own roundings may add instead of averaging.
# Were the kernel's deviation from the emulation as large as the emulation's own error AND fully correlated with it, the distance to
# the exact result would double: margin 2.  (Independent, it would be sqrt 2.)  Nothing here is taken from the code under test.
EMBED_MARGIN = 2.0


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


def embed_bar(cn_sd, hint, exact=None):
    exact = embed_ref(cn_sd, hint) if exact is None else exact
    return EMBED_MARGIN * rel_l2(embed_ref(cn_sd, hint, emulate=True), exact)


# ---------------------------------------------------------------------------------------------------------------- the residual add
ADD_CASES = ((3, 24, 32), (2, 1008, 320), (7, 64, 1280))          # (B, HW, C)


def add_inputs(B, HW, C, n, seed=0):
    """skip fp16 [B, HW, C] with trunk-sized values, r fp32 [n, HW, C] of the same size (and a few large / tiny ones: both roundings
    are exercised across binades)."""
    g = torch.Generator().manual_seed(1000 * B + HW + C + seed)
    skip = (torch.randn(B, HW, C, generator=g) * 2).half()
    r = torch.randn(n, HW, C, generator=g) * torch.exp2(torch.randint(-6, 4, (n, HW, 1), generator=g).float())
    return skip, r


def add_ref(skip, r, streams, scales):
    """fp64: out[b] = skip[b] + fp32(scale_i) r[i] for b = streams[i], every other stream unchanged; and the bar of
    skip[b] <- f16(fmaf(scale, r, float(skip))) per element:
        one fp32 rounding of the exact fma      <= 2^-24 |v|
        one fp16 rounding of that fp32 value    <= 2^-11 |v| (1 + 2^-24)   normal range;  <= 2^-25 absolute below 2^-14 (fp16 subnormals)
    v = the exact value.  Untouched streams have bar 0 (they keep their bytes)."""
    out = skip.double().clone()
    bar = torch.zeros_like(out)
    for i, b in enumerate(streams):
        s = float(torch.tensor(float(scales[i]), dtype=torch.float32))
        v = skip[b].double() + s * r[i].double()
        out[b] = v
        bar[b] = 2.0 ** -24 * v.abs() + 2.0 ** -11 * v.abs() * (1 + 2.0 ** -24) + 2.0 ** -25
    return out, bar


# ---------------------------------------------------------------------------------------------------------------- the forward
class ControlOracleUNet(OracleUNet):
    """OracleUNet + one ControlNet (keys under "controlnet." in the same state dict).  The k-th forward() call (of batch 1) carries
    schedule[k] = the conditioning scale of that stream (0 / None = not controlled: the plain forward), so that
    freeu_ref.oracle_streams and oracle.region_loop.rich_step_forwards run their streams each with the scale of the prompt it runs.
    `hint`: [Ch, 8 h, 8 w].  The control copy sees no font size, no capture / injection and no token-map store; a trace records its
    modules under "controlnet.<module>", the embedding under "controlnet.hint_embedding", and the main UNet's skips / mid output after
    the add under "controlnet.skip.{k}" / "controlnet.mid".
    `fault`: "embedding_on_unet_conv_in" adds the hint embedding to the main UNet's conv_in output instead of the control copy's (the
    wrong side of conv_in); "no_residuals" drops the adds - for the discrimination checks."""

    def __init__(self, config, state_dict, cn_state_dict, hint, schedule, fault=None):
        sd = dict(state_dict)
        sd.update(prefixed(cn_state_dict))
        super().__init__(config, sd)
        self.cn_sd = {k: v.detach().float() for k, v in cn_state_dict.items()}
        self.hint, self.schedule, self.calls, self.fault = hint, list(schedule), 0, fault
        self._emb = None

    def hint_embedding(self):
        if self._emb is None:
            self._emb = embed_ref(self.cn_sd, self.hint).float()[None]
        return self._emb

    def _emb_t(self, prefix, t, B, added):
        c = self.cfg
        emb = timestep_embedding(torch.as_tensor(t).reshape(-1).expand(B), c["block_out_channels"][0])
        emb = self._lin(F.silu(self._lin(emb, prefix + "time_embedding.linear_1")), prefix + "time_embedding.linear_2")
        if c["addition_embed_type"] == "text_time":
            tid = timestep_embedding(added["time_ids"].flatten(), c["addition_time_embed_dim"]).reshape(added["text_embeds"].shape[0], -1)
            add = torch.cat([added["text_embeds"].float(), tid], dim=-1)
            emb = emb + self._lin(F.silu(self._lin(add, prefix + "add_embedding.linear_1")), prefix + "add_embedding.linear_2")
        return emb

    def control_residuals(self, sample, timestep, ctx, added, scale, trace=None):
        """ControlNetModel.forward -> ([residual per skip], mid residual), scaled."""
        c = self.cfg
        boc, nlev = c["block_out_channels"], len(c["block_out_channels"])

        def rec(name, x):
            if trace is not None:
                trace[P + name] = x.detach()
        emb = self._emb_t(P, timestep, sample.shape[0], added)
        x = self._conv(sample.float(), P + "conv_in")
        if self.fault != "embedding_on_unet_conv_in":
            x = x + self.hint_embedding()
        rec("conv_in", x)
        skips = [x]
        for i, bt in enumerate(c["down_block_types"]):
            for j in range(c["layers_per_block"][i]):
                x = self._resnet(f"{P}down_blocks.{i}.resnets.{j}", x, emb, None)
                rec(f"down_blocks.{i}.resnets.{j}", x)
                if bt == "CrossAttnDownBlock2D":
                    x = self._transformer(f"{P}down_blocks.{i}.attentions.{j}", x, ctx, c["attention_head_dim"][i], c["transformer_layers_per_block"][i], None)
                    rec(f"down_blocks.{i}.attentions.{j}", x)
                skips.append(x)
            if i != nlev - 1:
                x = self._conv(x, f"{P}down_blocks.{i}.downsamplers.0.conv", stride=2, padding=1)
                rec(f"down_blocks.{i}.downsamplers.0.conv", x)
                skips.append(x)
        x = self._resnet(P + "mid_block.resnets.0", x, emb, None)
        rec("mid_block.resnets.0", x)
        x = self._transformer(P + "mid_block.attentions.0", x, ctx, c["attention_head_dim"][-1], c["transformer_layers_per_block"][-1], None)
        rec("mid_block.attentions.0", x)
        x = self._resnet(P + "mid_block.resnets.1", x, emb, None)
        rec("mid_block.resnets.1", x)
        down = [scale * self._conv(s, f"{P}controlnet_down_blocks.{k}", padding=0) for k, s in enumerate(skips)]
        return down, scale * self._conv(x, P + "controlnet_mid_block", padding=0)

    def forward(self, sample, timestep, ctx, added=None, ctl=None, store=None):
        scale = self.schedule[self.calls % len(self.schedule)]
        self.calls += 1
        if not scale:
            return super().forward(sample, timestep, ctx, added, ctl, store)
        trace = ctl.get("trace") if ctl else None
        down, mid_r = self.control_residuals(sample, timestep, ctx, added, float(scale), trace)
        if trace is not None:
            trace[P + "hint_embedding"] = self.hint_embedding()
        if self.fault == "no_residuals":
            down, mid_r = [torch.zeros_like(d) for d in down], torch.zeros_like(mid_r)
        # UNet2DConditionModel.forward with the residuals: OracleUNet.forward restated op for op (oracle/unet.py), the adds behind the
        # down path and behind the mid block
        c = self.cfg
        boc, nlev = c["block_out_channels"], len(c["block_out_channels"])
        emb = self._emb_t("", timestep, sample.shape[0], added)
        x = self._conv(sample.float(), "conv_in")
        if self.fault == "embedding_on_unet_conv_in":
            x = x + self.hint_embedding()
        self._trace(ctl, "conv_in", x)
        skips = [x]
        for i, bt in enumerate(c["down_block_types"]):
            heads = c["attention_head_dim"][i]
            for j in range(c["layers_per_block"][i]):
                x = self._resnet(f"down_blocks.{i}.resnets.{j}", x, emb, ctl)
                self._trace(ctl, f"down_blocks.{i}.resnets.{j}", x)
                if bt == "CrossAttnDownBlock2D":
                    x = self._transformer(f"down_blocks.{i}.attentions.{j}", x, ctx, heads, c["transformer_layers_per_block"][i], ctl, store)
                    self._trace(ctl, f"down_blocks.{i}.attentions.{j}", x)
                skips.append(x)
            if i != nlev - 1:
                x = self._conv(x, f"down_blocks.{i}.downsamplers.0.conv", stride=2, padding=1)
                self._trace(ctl, f"down_blocks.{i}.downsamplers.0.conv", x)
                skips.append(x)
        heads = c["attention_head_dim"][-1]
        x = self._resnet("mid_block.resnets.0", x, emb, ctl)
        self._trace(ctl, "mid_block.resnets.0", x)
        x = self._transformer("mid_block.attentions.0", x, ctx, heads, c["transformer_layers_per_block"][-1], ctl, store)
        self._trace(ctl, "mid_block.attentions.0", x)
        x = self._resnet("mid_block.resnets.1", x, emb, ctl)
        self._trace(ctl, "mid_block.resnets.1", x)
        assert len(down) == len(skips)
        skips = [s + d for s, d in zip(skips, down)]
        x = x + mid_r
        if trace is not None:
            for k, s in enumerate(skips):
                trace[f"{P}skip.{k}"] = s.detach()
            trace[P + "mid"] = x.detach()
        rev_heads = list(reversed(c["attention_head_dim"]))
        rev_tl = list(reversed(c["transformer_layers_per_block"]))
        rev_lpb = list(reversed(c["layers_per_block"]))
        for i, bt in enumerate(c["up_block_types"]):
            for j in range(rev_lpb[i] + 1):
                x = torch.cat([x, skips.pop()], dim=1)
                x = self._resnet(f"up_blocks.{i}.resnets.{j}", x, emb, ctl)
                self._trace(ctl, f"up_blocks.{i}.resnets.{j}", x)
                if bt == "CrossAttnUpBlock2D":
                    x = self._transformer(f"up_blocks.{i}.attentions.{j}", x, ctx, rev_heads[i], rev_tl[i], ctl, store)
                    self._trace(ctl, f"up_blocks.{i}.attentions.{j}", x)
            if i != nlev - 1:
                x = F.interpolate(x, scale_factor=2.0, mode="nearest")
                x = self._conv(x, f"up_blocks.{i}.upsamplers.0.conv")
                self._trace(ctl, f"up_blocks.{i}.upsamplers.0.conv", x)
        x = F.silu(self._gn(x, "conv_norm_out", c["norm_eps"]))
        x = self._conv(x, "conv_out")
        self._trace(ctl, "conv_out", x)
        return x


# the forward cases of tests/test_controlnet*.py: freeu_ref.forward_case's streams [uncond (slot 0), base + font size (slot 2), text_ref
# (slot 2), injected region (slot 1)] with the scales base 1.0 / region 0.5 / uncond 0 per prompt slot
FORWARD_SLOT_SCALES = (0.0, 0.5, 1.0)
FORWARD_STREAM_SLOTS = (0, 2, 2, 1)
FORWARD_STREAM_SCALES = tuple(FORWARD_SLOT_SCALES[s] for s in FORWARD_STREAM_SLOTS)


def control_case(which):
    """freeu_ref.forward_case + a synthetic ControlNet and a hint."""
    from freeu_ref import forward_case
    c = dict(forward_case(which))
    c["cn"] = control_state_dict(c["cfg"], seed=21)
    c["hint"] = make_hint(c["h"], c["w"])
    c["sd_cn"] = {**c["sd"], **prefixed(c["cn"])}
    return c


def traced_streams(o, c):
    """freeu_ref.oracle_streams with a trace per stream: ([out per stream], [trace dict per stream])."""
    from oracle.unet import INJECT_RESNET

    def added(k):
        return {"text_embeds": c["pooled"][k:k + 1], "time_ids": c["tid"]} if c["xl"] else None
    emb, t = c["emb"], c["t"]
    tr = [{}, {}, {}, {}]
    with torch.no_grad():
        r0 = o.forward(c["lat"], t, emb[:1], added(0), ctl={"trace": tr[0]})
        r1 = o.forward(c["lat"], t, emb[2:3], added(2), ctl={"fontsize": {"word_pos": c["wp"], "font_size": c["fs"]}, "trace": tr[1]})
        cap = {}
        r2 = o.forward(c["lat_ref"], t, emb[2:3], added(2), ctl={"capture": cap, "trace": tr[2]})
        inj = {k: v for k, v in cap.items() if k.endswith("attn1") or k == INJECT_RESNET}
        r3 = o.forward(c["lat"], t, emb[1:2], added(1), ctl={"inject": inj, "trace": tr[3]})
    return [r0[0], r1[0], r2[0], r3[0]], tr


# ---------------------------------------------------------------------------------------------------------------- steps and off-is-off
STEP_SLOT_SCALES = (0.7, 0.5, 0.0, 1.0)          # prompt slots [negative, region 0, region 1, base] of rich_case(): one region is not controlled


def rich_case(hw=32, R_=3, steps=3, seed=77):
    """A tiny-XL rich-text request (the one of tests/test_ip_adapter_gpu.py) + a synthetic ControlNet and a hint."""
    from oracle.schedulers import OracleEuler
    from oracle.unet import TINY_XL_CONFIG, random_state_dict
    cfg = TINY_XL_CONFIG
    g = torch.Generator().manual_seed(seed)
    sched = OracleEuler(); sched.set_timesteps(steps)
    sd = random_state_dict(cfg, seed=12)
    D = cfg["cross_attention_dim"]
    c = dict(cfg=cfg, sd=sd, hw=hw, steps=steps, sched=sched,
             emb=torch.randn(R_ + 1, 77, D, generator=g), pooled=torch.randn(R_ + 1, 32, generator=g),
             tid=torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]]),
             masks=torch.softmax(torch.randn(R_, 1, hw, hw, generator=g) * 2, 0).repeat(1, 4, 1, 1),
             lat=torch.randn(1, 4, hw, hw, generator=g) * sched.init_noise_sigma, gs=5.0, isa=0.5, ibg=0.4)
    c["cn"] = control_state_dict(cfg, seed=22)
    c["sd_cn"] = {**sd, **prefixed(c["cn"])}
    c["hint"] = make_hint(hw, hw, seed=6)
    return c


def _digest(t):
    import hashlib
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def off_digests(make_engine, after_prompts=None, device="cuda:0"):
    """sha256 of the outputs of the tiny forwards (freeu_ref.forward_case, the four stream modes) and of one injected region step
    (rich_case) on engines from make_engine(cfg, h, w, unet_state_dict) - which the caller closes through the returned engine's close();
    after_prompts(eng, case) runs behind set_prompts (the hook for "a hint but all scales 0").  Uses nothing a tree without a ControlNet
    lacks: tests/golden/controlnet_off_bits.json was recorded by this function on the commit before the ControlNet existed."""
    from freeu_ref import forward_case
    out = {}
    for which in ("xl", "sd"):
        c = forward_case(which)
        eng = make_engine(c["cfg"], c["h"], c["w"], c["sd"])
        try:
            if c["xl"]:
                eng.set_prompts(c["emb"].to(device), c["pooled"].to(device), c["tid"])
            else:
                eng.set_prompts(c["emb"].to(device))
            eng.set_fontsize(c["wp"], c["fs"])
            if after_prompts is not None:
                after_prompts(eng, c)
            x = torch.cat([c["lat"], c["lat"], c["lat_ref"], c["lat"]]).to(device)
            out[f"forward_{which}"] = _digest(eng.unet_forward(x, c["t"], [0, 2, 2, 1], fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2]))
        finally:
            eng.close()
    c = rich_case()
    c["h"] = c["w"] = c["hw"]
    eng = make_engine(c["cfg"], c["hw"], c["hw"], c["sd"])
    try:
        eng.set_prompts(c["emb"].to(device), c["pooled"].to(device), c["tid"])
        if after_prompts is not None:
            after_prompts(eng, c)
        eng.set_masks(c["masks"].to(device))
        eng.set_fontsize(torch.tensor([3, 5]), torch.tensor([4.0, -2.0]))
        eng.set_schedule(0, c["sched"].timesteps.tolist(), c["sched"].sigmas.tolist(), c["steps"])
        eng.set_latents(c["lat"].to(device))
        eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
        lat, ref = eng.read_latents(c["hw"], c["hw"], with_ref=True)
        out["region_step_latents"], out["region_step_reference_latents"] = _digest(lat), _digest(ref)
    finally:
        eng.close()
    return out
