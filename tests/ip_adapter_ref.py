"""References for image prompts by decoupled cross-attention (IP-Adapter; csrc/ipattn.hip, include/rtdiff.h: rt_set_image_prompts /
rt_op_ip_attention).  Test infrastructure, plain torch.  The formulas are [memory] of diffusers' IPAdapterAttnProcessor / ImageProjection
and of the original IP-Adapter checkpoint layout; the reference project has no counterpart, so parity is unpinned and these tests pin
the restatements below instead.

  op_inputs / op_ref      the inputs of the op tests (bf16 values, the engine's padded layouts) and the fp64 restatement of the op
                          O + sigma softmax_2(Q Kip^T) Vip over the first T keys, with the per-element bar
  emulate                 a CPU emulation of an honest kernel (fp32 scores, exp2, P to bf16, fp32 PV, one rounding) and of three faulty
                          ones - tests/test_ip_adapter.py proves the bar passes the first and catches the others
  ip_attn_impl            plugs into OracleUNet.attn_impl: the image term on attn2 only, per batch entry
  IpOracleUNet            an OracleUNet whose successive forward() calls take their image from a schedule (for freeu_ref.oracle_streams)
  diffusers_processor     the direct restatement of diffusers' IPAdapterAttnProcessor.__call__ for ONE global image
  ip_weights              to_k_ip / to_v_ip of every attn2 from random_state_dict's uniform(+-1 / sqrt(fan_in)) family
  synthetic_checkpoint    an IP-Adapter checkpoint in the original layout (image_proj.* / ip_adapter.*) for a UNet config

THE OP BAR (derived, not measured), per output element:
    bar = 2^-8 |ref| + 2^-7 |sigma| sum_j p_j |v_j| + 2^-14 (|O_in| + |sigma| sum_j p_j |v_j|)
  first term: the ONE final rounding to bf16 (half an ulp); second: P rounded to bf16 for the PV product - 2^-8 at worst, doubled because
  a kernel may normalise by the sum of the rounded or of the unrounded exponentials; third: fp32 accumulation and second-order effects."""
import math

import torch

from oracle.unet import OracleUNet, attention_probs

# (N, H, d, DP, T): the shapes of the op test - one tile with 8 queries, head dims below and at every padded width, a tail tile (24, 80,
# 1008 = 63 tiles: the last run of tiles of a wave is short), T = 1, a count that is no multiple of 4, all 16 keys
OP_CASES = ((8, 1, 8, 32, 1), (24, 5, 40, 64, 4), (24, 3, 80, 96, 3), (80, 2, 64, 64, 16), (64, 1, 160, 160, 16), (1008, 2, 64, 64, 4))
OP_SLOTS = (1, -1, 0)
OP_SCALES = (0.6, 0.0, -0.5)
NSLOT = 2


def bf(x):
    return x.to(torch.bfloat16)


def op_inputs(N, H, d, DP, T, B=3, nslot=NSLOT, gain=2.0, seed=None):
    """Q, O [B, N, H, DP], K [nslot, 16, H, DP], V [nslot, 16, H, DP] as bf16 values on the CPU.  Q is drawn at `gain` times the unit score
    gain and carries d^-1/2 log2 e; columns d .. DP of Q, K and V are zero (what the engine's packed projections leave), O's hold data;
    key rows T .. 15 of K and V hold LARGE values, not zeros: a kernel that scores them instead of masking them is far off."""
    g = torch.Generator().manual_seed(N * 131 + d * 7 + T if seed is None else seed)
    Q = torch.zeros(B, N, H, DP); K = torch.zeros(nslot, 16, H, DP); V = torch.zeros(nslot, 16, H, DP)
    Q[..., :d] = torch.randn(B, N, H, d, generator=g) * gain * d ** -0.5 * math.log2(math.e)
    K[..., :d] = torch.randn(nslot, 16, H, d, generator=g)
    V[..., :d] = torch.randn(nslot, 16, H, d, generator=g)
    K[:, T:, :, :d] *= 4.0
    V[:, T:, :, :d] += 8.0
    O = torch.randn(B, N, H, DP, generator=g)
    return bf(Q), bf(K), bf(V), bf(O)


def op_ref(Q, K, V, O, slots, counts, scales):
    """fp64 restatement on the bf16 values -> (ref, bar), both [B, N, H, DP]; a skipped entry (slot < 0 or scale 0) is O itself, bar 0."""
    Q, K, V, O = Q.double(), K.double(), V.double(), O.double()
    ref, bar = O.clone(), torch.zeros_like(O)
    for b, (s, T, sg) in enumerate(zip(slots, counts, scales)):
        if s < 0 or sg == 0:
            continue
        sc = torch.einsum("nhd,thd->nht", Q[b], K[s, :T])
        p = torch.softmax(sc * math.log(2.0), -1)                     # base-2 exponent: Q carries log2 e
        ip = torch.einsum("nht,thd->nhd", p, V[s, :T])
        aip = torch.einsum("nht,thd->nhd", p, V[s, :T].abs())
        ref[b] = O[b] + sg * ip
        bar[b] = 2.0 ** -8 * ref[b].abs() + 2.0 ** -7 * abs(sg) * aip + 2.0 ** -14 * (O[b].abs() + abs(sg) * aip)
    return ref, bar


def emulate(Q, K, V, O, slots, counts, scales, *, extra_keys=0, scale_err=1.0, drop_term=False):
    """An honest kernel on the CPU: fp32 scores, exp2 against the row maximum, P rounded to bf16 unnormalised, fp32 PV, divided by the
    fp32 sum of the unrounded exponentials, one fma into fp32(O), ONE rounding to bf16.  Mutations: extra_keys = that many pad keys (the
    cached rows behind the count, as zero rows would be: score 0, value 0) scored instead of masked; scale_err = the scale off by that
    factor; drop_term = the image term missing."""
    out = O.clone()
    for b, (s, T, sg) in enumerate(zip(slots, counts, scales)):
        if s < 0 or sg == 0 or drop_term:
            continue
        sc = torch.einsum("nhd,thd->nht", Q[b].float(), K[s, :T].float())
        v = V[s, :T].float()
        if extra_keys:
            sc = torch.cat([sc, torch.zeros(*sc.shape[:2], extra_keys)], -1)
            v = torch.cat([v, torch.zeros(extra_keys, *v.shape[1:])], 0)
        e = torch.exp2(sc - sc.max(-1, keepdim=True).values)
        ip = torch.einsum("nht,thd->nhd", bf(e).float(), v) / e.sum(-1, keepdim=True)
        out[b] = bf(O[b].float() + float(sg * scale_err) * ip)
    return out


def worst_and_share(got, ref, bar):
    """(largest |got - ref| / bar, share of elements above 1) over the elements with a bar (the launched entries)."""
    m = bar > 0
    ratio = (got.double() - ref).abs()[m] / bar[m]
    return ratio.max().item(), (ratio > 1).double().mean().item()


# ---------------------------------------------------------------------------------------------------------------- the oracle
def ip_weights(sd, seed):
    """to_k_ip / to_v_ip for every attn2 of state dict `sd`, uniform(+-1 / sqrt(fan_in)) like random_state_dict."""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, v in sd.items():
        if k.endswith(".attn2.to_k.weight"):
            b = 1.0 / math.sqrt(v.shape[1])
            out[k.replace("to_k.weight", "to_k_ip.weight")] = (torch.rand(v.shape, generator=g) * 2 - 1) * b
            out[k.replace("to_k.weight", "to_v_ip.weight")] = (torch.rand(v.shape, generator=g) * 2 - 1) * b
    return out


def ip_attn_impl(tokens_per_entry, scale_per_entry):
    """-> attn_impl for OracleUNet: OracleUNet._attention, plus on attn2 (ctx given) for batch entry b with tokens_per_entry[b] ([t, D] or
    None) and scale_per_entry[b] != 0 the term scale softmax(q k_ip^T d^-1/2) v_ip added to the attention output in front of to_out."""
    def impl(o, name, x, heads, ctx, fontsize, real_probs):
        B, N, C = x.shape
        q = o._lin(x, name + ".to_q", bias=False)
        src = x if ctx is None else ctx
        k = o._lin(src, name + ".to_k", bias=False)
        v = o._lin(src, name + ".to_v", bias=False)
        d = C // heads

        def h2b(t):
            return t.reshape(t.shape[0], -1, heads, d).permute(0, 2, 1, 3).reshape(t.shape[0] * heads, -1, d)
        q, k, v = h2b(q), h2b(k), h2b(v)
        probs = attention_probs(q, k, d ** -0.5, fontsize) if real_probs is None else real_probs
        out = torch.bmm(probs, v)
        if ctx is not None:
            assert len(tokens_per_entry) == B and len(scale_per_entry) == B, (len(tokens_per_entry), B)
            for b in range(B):
                tk, sg = tokens_per_entry[b], scale_per_entry[b]
                if tk is None or sg == 0:
                    continue
                tk = tk.to(x.dtype)[None]
                kip = h2b(o._lin(tk, name + ".to_k_ip", bias=False))
                vip = h2b(o._lin(tk, name + ".to_v_ip", bias=False))
                qb = q[b * heads:(b + 1) * heads]
                p = torch.softmax(torch.bmm(qb, kip.transpose(1, 2)) * d ** -0.5, -1)
                out = out.clone()
                out[b * heads:(b + 1) * heads] = out[b * heads:(b + 1) * heads] + sg * torch.bmm(p, vip)
        out = out.reshape(B, heads, N, d).permute(0, 2, 1, 3).reshape(B, N, C)
        return o._lin(out, name + ".to_out.0"), probs
    return impl


class IpOracleUNet(OracleUNet):
    """OracleUNet whose k-th forward() call (of batch 1) carries schedule[k] = (tokens [t, D] or None, scale): lets
    freeu_ref.oracle_streams run its four streams, each with the image of the prompt it runs."""

    def __init__(self, config, state_dict, schedule):
        super().__init__(config, state_dict)
        self.schedule, self.calls = list(schedule), 0

    def forward(self, sample, timestep, ctx, added=None, ctl=None, store=None):
        tk, sg = self.schedule[self.calls]
        self.calls += 1
        self.attn_impl = ip_attn_impl([tk] * sample.shape[0], [sg] * sample.shape[0])
        try:
            return super().forward(sample, timestep, ctx, added, ctl, store)
        finally:
            self.attn_impl = None


def diffusers_processor(sd, name, heads, hidden, text, ip_tokens, scale):
    """diffusers' IPAdapterAttnProcessor.__call__ ([memory]) for one image, in the dtype of its inputs: hidden [B, N, C], text [B, 77, D],
    ip_tokens [B, t, D];  hidden_states = attn(q, k, v) + scale * attn(q, to_k_ip(ip), to_v_ip(ip)), then to_out."""
    W = {k: sd[f"{name}.{k}.weight"].to(hidden.dtype) for k in ("to_q", "to_k", "to_v", "to_k_ip", "to_v_ip", "to_out.0")}
    B, N, C = hidden.shape
    d = C // heads

    def heads_first(t):
        return t.reshape(B, -1, heads, d).transpose(1, 2)

    def attn(q, k, v):
        return torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(d), -1) @ v
    q = heads_first(hidden @ W["to_q"].T)
    hs = attn(q, heads_first(text @ W["to_k"].T), heads_first(text @ W["to_v"].T))
    ip = attn(q, heads_first(ip_tokens @ W["to_k_ip"].T), heads_first(ip_tokens @ W["to_v_ip"].T))
    hs = (hs + scale * ip).transpose(1, 2).reshape(B, N, C)
    return hs @ W["to_out.0"].T + sd[f"{name}.to_out.0.bias"].to(hidden.dtype)


# ---------------------------------------------------------------------------------------------------------------- checkpoints
def attn2_names(cfg):
    """The attn2 modules of a UNet config in the order of the reference UNet's attn_processors: down blocks, up blocks, mid block."""
    n = len(cfg["block_out_channels"])

    def tup(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v,) * n
    lpb, tl = tup(cfg["layers_per_block"]), tup(cfg["transformer_layers_per_block"])
    out = []
    for i, bt in enumerate(cfg["down_block_types"]):
        if bt == "CrossAttnDownBlock2D":
            out += [f"down_blocks.{i}.attentions.{j}.transformer_blocks.{k}.attn2" for j in range(lpb[i]) for k in range(tl[i])]
    for i, bt in enumerate(cfg["up_block_types"]):
        if bt == "CrossAttnUpBlock2D":
            out += [f"up_blocks.{i}.attentions.{j}.transformer_blocks.{k}.attn2" for j in range(lpb[n - 1 - i] + 1) for k in range(tl[n - 1 - i])]
    out += [f"mid_block.attentions.0.transformer_blocks.{k}.attn2" for k in range(tl[n - 1])]
    return out


def synthetic_checkpoint(cfg, sd, T=4, E=24, seed=9, layout="original"):
    """An IP-Adapter checkpoint for `cfg`: image_proj (ImageProjection: proj [T D, E] + LayerNorm(D)) and the per-layer projections, as
    flat keys of the original layout (ip_adapter.{2k+1}.to_k_ip.weight), the nested dict, or diffusers' processor names.  The layer
    weights are ip_weights(sd, seed)'s, so -> (checkpoint, the engine-named weights the loader must return)."""
    D = cfg["cross_attention_dim"]
    g = torch.Generator().manual_seed(seed + 1)
    proj = {"proj.weight": (torch.rand(T * D, E, generator=g) * 2 - 1) / math.sqrt(E), "proj.bias": 0.05 * (torch.rand(T * D, generator=g) * 2 - 1),
            "norm.weight": 1.0 + 0.1 * (torch.rand(D, generator=g) * 2 - 1), "norm.bias": 0.05 * (torch.rand(D, generator=g) * 2 - 1)}
    want = ip_weights(sd, seed)
    layers = {}
    for k, name in enumerate(attn2_names(cfg)):
        for w in ("to_k_ip", "to_v_ip"):
            key = f"{name}.processor.{w}.0.weight" if layout == "diffusers" else f"{2 * k + 1}.{w}.weight"
            layers[key] = want[f"{name}.{w}.weight"]
    if layout == "nested":
        return {"image_proj": proj, "ip_adapter": layers}, want
    ck = {f"image_proj.{k}": v for k, v in proj.items()}
    ck.update({(k if layout == "diffusers" else f"ip_adapter.{k}"): v for k, v in layers.items()})
    return ck, want


def project_ref(proj, embeds):
    """ImageProjection in fp64: LayerNorm(Linear(e).reshape(T, D)).  embeds [E] -> [T, D]."""
    D = proj["norm.weight"].shape[0]
    y = (proj["proj.weight"].double() @ embeds.double() + proj["proj.bias"].double()).reshape(-1, D)
    return torch.nn.functional.layer_norm(y, (D,), proj["norm.weight"].double(), proj["norm.bias"].double(), 1e-5)
