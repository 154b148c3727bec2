"""References for the Resampler of the IP-Adapter "plus" checkpoints (csrc/resampler.hip, include/rtdiff.h: rt_op_latent_attention;
rich_text_to_image_amd/resampler.py).  Test infrastructure, plain torch.  The Resampler's formulas are [memory] of the IP-Adapter
repository's resampler.py; the reference project has no counterpart, so these tests pin the restatements below.

  attn_inputs / attn_ref   the inputs of the attention tests (bf16 values: q [B Nq, H d], kv [B Nk, 2 H d] = k | v per row) and the fp64
                           restatement softmax(scale Q K^T) V with the per-element bar
  emulate                  a CPU emulation of an honest split-key kernel - wave w of four takes the key tiles w, w + 4, ... of 64 keys with
                           its own running (m, l, O); fp32 scores times scale log2 e, P rounded to bf16 against the running maximum, fp32
                           PV; the partial results merged in wave order with f_w = exp2(m_w - M) (0 for a wave without keys), one division
                           and one rounding - and of five faulty ones; tests/test_resampler.py proves the bar passes the first and catches
                           the others
  resampler_ref            Resampler.forward in fp64 (or any dtype) on the given weights
  resampler_emulate        the chain of resampler.py with its bf16 roundings, on the CPU
  random_resampler / synthetic_plus_checkpoint     random weights under the checkpoint's key names; a whole plus adapter for a UNet config

THE ATTENTION BAR is tests/clip_vision_ref.py's, unchanged, per output element:
    bar = 2^-8 |ref| + (2^-7 + 2^-14) sum_j p_j |v_j|
  Its third term allows ten rescalings by exp2(m_old - m_new); a wave here makes at most three (11 key tiles over four waves) and the merge
  adds four."""
import math

import torch

import ip_adapter_ref as R

# (B, H, Nq, Nk, d)
ATTN_CASES = ((1, 1, 1, 1, 8),            # three waves without a key
              (1, 2, 16, 17, 64),         # less than one key tile
              (1, 3, 8, 25, 80),          # fewer than 16 queries, head dim padded
              (2, 1, 4, 65, 104),         # one key past a tile
              (2, 2, 16, 273, 64),        # the shipping shape: 4 tiles and 17 keys
              (1, 2, 16, 656, 64),        # the limit
              (1, 20, 16, 273, 64))       # SDXL's head count
KEY_TILE, WAVES = 64, 4
LOG2E = 1.44269504088896340736


def bf(x):
    return x.to(torch.bfloat16)


def padded(d):
    return -(-d // 32) * 32


def attn_inputs(B, H, Nq, Nk, d, gain=2.0, seed=None):
    """(q [B Nq, H d], kv [B Nk, 2 H d]) bf16 on the CPU, built like clip_vision_ref.attn_inputs: scores of standard deviation `gain`,
    every key with a common offset of 2 (the softmax does not see the shift it gives a query's scores, a kernel that scores a padding key
    next to them does), values offset by 0.5."""
    g = torch.Generator().manual_seed(Nk * 131 + d * 7 + H + 1009 * Nq if seed is None else seed)
    q = torch.randn(B * Nq, H, d, generator=g) * gain
    k = torch.randn(B * Nk, H, d, generator=g) + 2.0
    v = torch.randn(B * Nk, H, d, generator=g) + 0.5
    return bf(q.reshape(B * Nq, -1)), bf(torch.cat([k.reshape(B * Nk, -1), v.reshape(B * Nk, -1)], 1))


def split(q, kv, B, H, Nq, Nk, d):
    """-> q [B, H, Nq, d], k, v [B, H, Nk, d] as views of the values."""
    qq = q.reshape(B, Nq, H, d).permute(0, 2, 1, 3)
    k, v = (kv[:, i * H * d:(i + 1) * H * d].reshape(B, Nk, H, d).permute(0, 2, 1, 3) for i in range(2))
    return qq, k, v


def attn_ref(q, kv, B, H, Nq, Nk, d):
    """fp64 restatement on the bf16 values -> (ref, bar), both [B Nq, H d]."""
    qq, k, v = (t.double() for t in split(q, kv, B, H, Nq, Nk, d))
    p = torch.softmax(qq @ k.transpose(-1, -2) * d ** -0.5, -1)
    ref, apv = p @ v, p @ v.abs()
    bar = 2.0 ** -8 * ref.abs() + (2.0 ** -7 + 2.0 ** -14) * apv
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * Nq, H * d)
    return back(ref), back(bar)


def emulate(q, kv, B, H, Nq, Nk, d, *, pad_key=False, drop_last=False, no_factors=False, padded_scale=False, no_latent_keys=False):
    """An honest split-key kernel on the CPU (see the module docstring) -> bf16 [B Nq, H d].  Mutations: pad_key = the first padding key
    behind Nk (a zero row: score 0, value 0) scored instead of masked; drop_last = the last valid key masked; no_factors = the merge
    adds the waves' l and O without the exp2(m_w - M) factors; padded_scale = DP^-1/2 instead of d^-1/2; no_latent_keys = the last Nq
    keys (the latents' own rows in the Resampler) left out.  A mutation that leaves no key at all gives NaN."""
    qq, k, v = (t.float() for t in split(q, kv, B, H, Nq, Nk, d))
    sl = torch.tensor((padded(d) if padded_scale else d) ** -0.5 * LOG2E, dtype=torch.float32)
    if pad_key:
        k = torch.cat([k, torch.zeros(B, H, 1, d)], 2); v = torch.cat([v, torch.zeros(B, H, 1, d)], 2)
    if drop_last:
        k, v = k[:, :, :Nk - 1], v[:, :, :Nk - 1]
    if no_latent_keys:
        k, v = k[:, :, :Nk - Nq], v[:, :, :Nk - Nq]
    parts = []
    for w in range(WAVES):
        m = torch.full((B, H, Nq, 1), -float("inf")); l = torch.zeros(B, H, Nq, 1); o = torch.zeros(B, H, Nq, d)
        for k0 in range(w * KEY_TILE, k.shape[2], WAVES * KEY_TILE):
            s = (qq @ k[:, :, k0:k0 + KEY_TILE].transpose(-1, -2)) * sl
            mn = torch.maximum(m, s.max(-1, keepdim=True).values)
            alpha = torch.exp2(m - mn)
            p = torch.exp2(s - mn)
            l = l * alpha + p.sum(-1, keepdim=True)
            o = o * alpha + bf(p).float() @ v[:, :, k0:k0 + KEY_TILE]
            m = mn
        parts.append((m, l, o))
    M = torch.stack([p[0] for p in parts]).max(0).values
    L, O = torch.zeros(B, H, Nq, 1), torch.zeros(B, H, Nq, d)
    for m, l, o in parts:                                               # wave order 0, 1, 2, 3
        f = torch.where(torch.isinf(m), torch.zeros_like(m), torch.ones_like(m) if no_factors else torch.exp2(m - M))
        L = L + l * f
        O = O + o * f
    return bf((O / L).permute(0, 2, 1, 3).reshape(B * Nq, H * d))


def worst(got, ref, bar):
    """Largest |got - ref| / bar; a NaN anywhere counts as a failure (inf)."""
    r = (got.double() - ref).abs() / bar
    return float("inf") if bool(torch.isnan(r).any()) else r.max().item()


# ---------------------------------------------------------------------------------------------------------------- the Resampler
# (E, dim, dim_head, heads, T, depth, D, N, B): two small ones (odd sizes: 17 and 50 tokens, heads of 32 and of 8), one SD-v1.5 layer of
# ip-adapter-plus_sd15 and two layers of ip-adapter-plus_sdxl_vit-h at full width
GEOMETRIES = ((160, 128, 32, 4, 4, 2, 64, 17, 2), (208, 96, 8, 12, 16, 4, 48, 50, 1),
              (1280, 768, 64, 12, 16, 1, 768, 257, 1), (1280, 1280, 64, 20, 16, 2, 2048, 257, 1))
FF_MULT = 4


def random_resampler(E, dim, dim_head, heads, T, depth, D, seed=0, gain=1.0):
    """The tensors below image_proj. of a plus checkpoint: matrices N(0, 1 / fan_in) x gain, LayerNorm weights near 1, biases small,
    latents N(0, 1 / dim) (as the module initialises them)."""
    g = torch.Generator().manual_seed(seed)
    inner, ff = heads * dim_head, FF_MULT * dim
    mat = lambda o, i: torch.randn(o, i, generator=g) * (gain * i ** -0.5)
    ln_w = lambda n: 1 + 0.1 * torch.randn(n, generator=g)
    small = lambda n: 0.1 * torch.randn(n, generator=g)
    w = {"latents": torch.randn(1, T, dim, generator=g) * dim ** -0.5, "proj_in.weight": mat(dim, E), "proj_in.bias": small(dim),
         "proj_out.weight": mat(D, dim), "proj_out.bias": small(D), "norm_out.weight": ln_w(D), "norm_out.bias": small(D)}
    for i in range(depth):
        p = f"layers.{i}."
        w.update({p + "0.norm1.weight": ln_w(dim), p + "0.norm1.bias": small(dim), p + "0.norm2.weight": ln_w(dim), p + "0.norm2.bias": small(dim),
                  p + "0.to_q.weight": mat(inner, dim), p + "0.to_kv.weight": mat(2 * inner, dim), p + "0.to_out.weight": mat(dim, inner),
                  p + "1.0.weight": ln_w(dim), p + "1.0.bias": small(dim), p + "1.1.weight": mat(ff, dim), p + "1.3.weight": mat(dim, ff)})
    return w


def hidden_inputs(B, N, E, seed=0):
    """Hidden states like an encoder's trunk: unit-variance features with a per-feature offset."""
    g = torch.Generator().manual_seed(seed + 17 * N + E)
    return torch.randn(B, N, E, generator=g) + 0.5 * torch.randn(E, generator=g)


def _depth(w):
    return 1 + max(int(k.split(".")[1]) for k in w if k.startswith("layers."))


def resampler_ref(w, hidden, dim_head, dtype=torch.float64, no_latent_keys=False, swap_kv=False):
    """Resampler.forward ([memory], see resampler.py) -> [B, T, D] in `dtype`.  Mutations: no_latent_keys = keys are the image tokens
    only; swap_kv = the k and v halves of to_kv exchanged."""
    W = {k: v.to(dtype) for k, v in w.items()}
    ln = lambda x, p: torch.nn.functional.layer_norm(x, (x.shape[-1],), W[p + ".weight"], W[p + ".bias"], 1e-5)
    h = hidden.to(dtype)
    B = h.shape[0]
    x = h @ W["proj_in.weight"].T + W["proj_in.bias"]
    lat = W["latents"].repeat(B, 1, 1)
    T = lat.shape[1]
    for i in range(_depth(w)):
        p = f"layers.{i}."
        xn, l2 = ln(x, p + "0.norm1"), ln(lat, p + "0.norm2")
        q = l2 @ W[p + "0.to_q.weight"].T
        kvin = xn if no_latent_keys else torch.cat([xn, l2], 1)
        k, v = (kvin @ W[p + "0.to_kv.weight"].T).chunk(2, -1)
        if swap_kv:
            k, v = v, k
        heads = q.shape[-1] // dim_head
        hd = lambda t: t.reshape(B, t.shape[1], heads, dim_head).transpose(1, 2)
        a = torch.softmax(hd(q) @ hd(k).transpose(-1, -2) * dim_head ** -0.5, -1) @ hd(v)
        lat = a.transpose(1, 2).reshape(B, T, -1) @ W[p + "0.to_out.weight"].T + lat
        f = torch.nn.functional.gelu(ln(lat, p + "1.0") @ W[p + "1.1.weight"].T)
        lat = f @ W[p + "1.3.weight"].T + lat
    return ln(lat @ W["proj_out.weight"].T + W["proj_out.bias"], "norm_out")


def resampler_emulate(w, hidden, dim_head, no_latent_keys=False, swap_kv=False):
    """resampler.py's chain on the CPU with its roundings: bf16 weights and GEMM operands, fp32 accumulation and trunk, LayerNorm / GELU /
    attention results rounded to bf16 (P rounded to bf16 for the PV product), the output rounded to bf16.  Same mutations as resampler_ref."""
    Wb = {k: bf(v).float() for k, v in w.items() if v.dim() == 2}
    ln = lambda x, p: bf(torch.nn.functional.layer_norm(x, (x.shape[-1],), w[p + ".weight"].float(), w[p + ".bias"].float(), 1e-5)).float()
    B = hidden.shape[0]
    x = bf(hidden.float()).float() @ Wb["proj_in.weight"].T + w["proj_in.bias"].float()
    lat = w["latents"].float().repeat(B, 1, 1)
    T = lat.shape[1]
    for i in range(_depth(w)):
        p = f"layers.{i}."
        xn, l2 = ln(x, p + "0.norm1"), ln(lat, p + "0.norm2")
        q = bf(l2 @ Wb[p + "0.to_q.weight"].T).float()
        kvin = xn if no_latent_keys else torch.cat([xn, l2], 1)
        k, v = bf(kvin @ Wb[p + "0.to_kv.weight"].T).float().chunk(2, -1)
        if swap_kv:
            k, v = v, k
        heads = q.shape[-1] // dim_head
        hd = lambda t: t.reshape(B, t.shape[1], heads, dim_head).transpose(1, 2)
        s = hd(q) @ hd(k).transpose(-1, -2) * dim_head ** -0.5
        e = torch.exp(s - s.max(-1, keepdim=True).values)
        a = bf(bf(e).float() @ hd(v) / e.sum(-1, keepdim=True)).float()
        lat = a.transpose(1, 2).reshape(B, T, -1) @ Wb[p + "0.to_out.weight"].T + lat
        f = bf(torch.nn.functional.gelu(bf(ln(lat, p + "1.0") @ Wb[p + "1.1.weight"].T).float())).float()
        lat = f @ Wb[p + "1.3.weight"].T + lat
    y = bf(lat).float() @ Wb["proj_out.weight"].T + w["proj_out.bias"].float()
    return ln(y, "norm_out")


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


def synthetic_plus_checkpoint(cfg, sd, E=160, dim=64, dim_head=64, heads=2, T=4, depth=2, seed=9, layout="original"):
    """A plus adapter for the UNet `cfg` (state dict `sd`): image_proj.* = random_resampler with D = cross_attention_dim, the per-layer
    projections ip_adapter_ref.ip_weights(sd, seed)'s, as flat keys of the original layout or the nested dict -> (checkpoint, the
    engine-named layer weights the loader must return, the image_proj tensors)."""
    D = cfg["cross_attention_dim"]
    proj = random_resampler(E, dim, dim_head, heads, T, depth, D, seed=seed + 2)
    want = R.ip_weights(sd, seed)
    layers = {f"{2 * k + 1}.{w}.weight": want[f"{name}.{w}.weight"] for k, name in enumerate(R.attn2_names(cfg)) for w in ("to_k_ip", "to_v_ip")}
    if layout == "nested":
        return {"image_proj": dict(proj), "ip_adapter": layers}, want, proj
    ck = {f"image_proj.{k}": v for k, v in proj.items()}
    ck.update({f"ip_adapter.{k}": v for k, v in layers.items()})
    return ck, want, proj
