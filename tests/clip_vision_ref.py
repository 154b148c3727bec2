"""References for the CLIP vision encoder's kernels (csrc/vision.hip; include/rtdiff.h: rt_op_patchify / rt_op_vit_embed /
rt_op_bidir_attention).  Test infrastructure, plain torch.

  attn_inputs / attn_ref   the inputs of the attention tests (bf16 values in the encoder's interleaved [B N, 3 H d] layout) and the fp64
                           restatement softmax(scale Q K^T) V with the per-element bar
  emulate                  a CPU emulation of an honest kernel - the kernel's own order: key tiles of 64, fp32 scores times scale log2 e,
                           running maximum and sum in fp32, P rounded to bf16 against the running maximum, fp32 PV, one division and one
                           rounding at the end - and of three faulty ones; tests/test_clip_vision.py proves the bar passes the first and
                           catches the others
  front_end_ref            patchify + patch convolution + class token + positions + pre-LayerNorm, directly, in fp64
  random_vision_model      transformers' CLIPVisionModelWithProjection with random weights (matrices x 3, as test_text_encoder_gpu.py)

THE ATTENTION BAR (derived, not measured), per output element - the form of ip_adapter_ref.py's op bar, for the same arithmetic class:
    bar = 2^-8 |ref| + 2^-7 sum_j p_j |v_j| + 2^-14 sum_j p_j |v_j|
  first term: the ONE final rounding to bf16 (half an ulp); second: P rounded to bf16 for the PV product - 2^-8 relative per probability
  whatever maximum it was taken against (the kernel rounds against the RUNNING maximum, which rescales p and its rounding error alike),
  doubled because a kernel may normalise by the sum of the rounded or of the unrounded exponentials; third: fp32 accumulation of the
  scores (|s| 2^-23 d per probability, |s| < 64 here), of P V over up to 640 keys and of the up to ten rescalings by exp2(m_old - m_new).
  The kernel's arithmetic differs from ipattn's in the online rescaling only, which the third term carries."""
import math

import torch

# (B, H, N, d): N = 257 is one past a multiple of 64 and of 32 (the last key tile holds ONE valid key), 17 and 50 are less than one tile,
# 577 = nine tiles and one key (ViT-L/14 at 336); 80 and 104 are the head dims that are padded (96, 128), 64 is not
ATTN_CASES = ((2, 2, 17, 80), (1, 2, 50, 104), (2, 4, 257, 64), (1, 16, 257, 80), (1, 3, 577, 104))
KEY_TILE = 64


def bf(x):
    return x.to(torch.bfloat16)


def padded(d):
    return -(-d // 32) * 32


def attn_inputs(B, H, N, d, gain=2.0, seed=None):
    """qkv [B N, 3 H d] bf16 on the CPU (q | k | v interleaved per row as the fused QKV GEMM leaves them).  Scores have standard deviation
    `gain`; every key carries a common offset, so that a query's scores share a shift of standard deviation 2 gain: the softmax does not
    see it, a kernel that scores a padding key (0) next to them does."""
    g = torch.Generator().manual_seed(N * 131 + d * 7 + H if seed is None else seed)
    q = torch.randn(B * N, H, d, generator=g) * gain
    k = torch.randn(B * N, H, d, generator=g) + 2.0
    v = torch.randn(B * N, H, d, generator=g) + 0.5
    return bf(torch.cat([q.reshape(B * N, -1), k.reshape(B * N, -1), v.reshape(B * N, -1)], 1))


def split(qkv, B, H, N, d):
    """-> q, k, v as [B, H, N, d] views of the values."""
    q, k, v = (qkv[:, i * H * d:(i + 1) * H * d].reshape(B, N, H, d).permute(0, 2, 1, 3) for i in range(3))
    return q, k, v


def attn_ref(qkv, B, H, N, d):
    """fp64 restatement on the bf16 values -> (ref, bar), both [B N, H d]."""
    q, k, v = (t.double() for t in split(qkv, B, H, N, d))
    p = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, -1)
    ref, apv = p @ v, p @ v.abs()
    bar = 2.0 ** -8 * ref.abs() + (2.0 ** -7 + 2.0 ** -14) * apv
    back = lambda t: t.permute(0, 2, 1, 3).reshape(B * N, H * d)
    return back(ref), back(bar)


def emulate(qkv, B, H, N, d, *, pad_key=False, drop_last=False, padded_scale=False):
    """An honest kernel on the CPU (see the module docstring) -> bf16 [B N, H d].  Mutations: pad_key = the first padding key behind N (a
    zero row: score 0, value 0) scored instead of masked; drop_last = the last valid key masked; padded_scale = DP^-1/2 instead of
    d^-1/2 (the padded head dim; the same kernel where d is a multiple of 32)."""
    q, k, v = (t.float() for t in split(qkv, B, H, N, d))
    sl = torch.tensor((padded(d) if padded_scale else d) ** -0.5 * 1.44269504088896340736, dtype=torch.float32)
    if pad_key:
        k = torch.cat([k, torch.zeros(B, H, 1, d)], 2); v = torch.cat([v, torch.zeros(B, H, 1, d)], 2)
    if drop_last:
        k, v = k[:, :, :N - 1], v[:, :, :N - 1]
    m = torch.full((B, H, N, 1), -float("inf")); l = torch.zeros(B, H, N, 1); o = torch.zeros(B, H, N, d)
    for k0 in range(0, k.shape[2], KEY_TILE):
        s = (q @ k[:, :, k0:k0 + KEY_TILE].transpose(-1, -2)) * sl
        mn = torch.maximum(m, s.max(-1, keepdim=True).values)
        alpha = torch.exp2(m - mn)
        p = torch.exp2(s - mn)
        l = l * alpha + p.sum(-1, keepdim=True)
        o = o * alpha + bf(p).float() @ v[:, :, k0:k0 + KEY_TILE]
        m = mn
    return bf((o / l).permute(0, 2, 1, 3).reshape(B * N, H * d))


def worst(got, ref, bar):
    return ((got.double() - ref).abs() / bar).max().item()


# ---------------------------------------------------------------------------------------------------------------- front end
CLIP_MEAN = (0.48145466, 0.4578275, 0.40821073)
CLIP_STD = (0.26862954, 0.26130258, 0.27577711)


def patch_rows_ref(px, p, Kp, mean=CLIP_MEAN, std=CLIP_STD):
    """uint8 [B, S, S, 3] -> fp64 [B (S/p)^2, Kp]: column (c p + ky) p + kx = (u / 255 - mean_c) / std_c, the padding columns zero."""
    B, S = px.shape[0], px.shape[1]
    G = S // p
    x = (px.double() / 255.0 - torch.tensor(mean, dtype=torch.float64)) / torch.tensor(std, dtype=torch.float64)      # [B, S, S, 3]
    x = x.reshape(B, G, p, G, p, 3).permute(0, 1, 3, 5, 2, 4).reshape(B * G * G, 3 * p * p)                           # (c, ky, kx)
    out = torch.zeros(B * G * G, Kp, dtype=torch.float64)
    out[:, :3 * p * p] = x
    return out


def front_end_ref(px, p, conv_w, cls, pos, gamma, beta, eps=1e-5):
    """The direct computation in fp64 on the values the kernels see (pixels normalised and rounded to bf16, the conv weight rounded to
    bf16): conv (stride p, no bias), class token, positions, LayerNorm -> [B N, C]."""
    B, S = px.shape[0], px.shape[1]
    G, Cc = S // p, conv_w.shape[0]
    x = (px.double() / 255.0 - torch.tensor(CLIP_MEAN, dtype=torch.float64)) / torch.tensor(CLIP_STD, dtype=torch.float64)
    x = bf(x.float()).double().permute(0, 3, 1, 2)                                                                     # [B, 3, S, S]
    y = torch.nn.functional.conv2d(x, bf(conv_w).double(), stride=p)                                                   # [B, C, G, G]
    y = y.flatten(2).transpose(1, 2)                                                                                   # [B, G G, C]
    e = torch.cat([cls.double().expand(B, 1, Cc), y], 1) + pos.double()[None]
    mu = e.mean(-1, keepdim=True)
    var = ((e - mu) ** 2).mean(-1, keepdim=True)
    return ((e - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()).reshape(B * (G * G + 1), Cc)


# ---------------------------------------------------------------------------------------------------------------- whole encoder
# (hidden, heads, layers, mlp, act, image, patch, proj)
ENCODER_CASES = ((160, 2, 3, 320, "quick_gelu", 56, 14, 48), (208, 2, 2, 416, "gelu", 98, 14, 64),
                 (1280, 16, 2, 5120, "gelu", 224, 14, 1024), (1664, 16, 1, 8192, "gelu", 224, 14, 1280))


def vision_config(case):
    hidden, heads, layers, mlp, act, image, patch, proj = case
    return dict(hidden_size=hidden, num_attention_heads=heads, num_hidden_layers=layers, intermediate_size=mlp, hidden_act=act,
                image_size=image, patch_size=patch, projection_dim=proj, layer_norm_eps=1e-5, num_channels=3)


def random_vision_model(case, seed=0):
    """transformers' CLIPVisionModelWithProjection, randomly initialised, every matrix scaled x 3 (attention far from uniform and
    activations in the non-linear range: the reason tests/test_text_encoder_gpu.py gives)."""
    from transformers import CLIPVisionConfig, CLIPVisionModelWithProjection
    torch.manual_seed(seed)
    model = CLIPVisionModelWithProjection(CLIPVisionConfig(**vision_config(case))).eval()
    with torch.no_grad():
        for n, prm in model.named_parameters():
            if prm.dim() >= 2 and "embedding" not in n:
                prm.mul_(3.0)
    return model


def synthetic_image(h, w, seed=0):
    """[h, w, 3] uint8: smooth gradients plus noise (a resize filter has something to do, a crop offset shows)."""
    g = torch.Generator().manual_seed(seed * 7 + h * 3 + w)
    yy, xx = torch.meshgrid(torch.arange(h, dtype=torch.float32), torch.arange(w, dtype=torch.float32), indexing="ij")
    base = torch.stack([xx / max(w - 1, 1), yy / max(h - 1, 1), (xx + yy) / max(h + w - 2, 1)], -1) * 200.0
    return (base + torch.rand(h, w, 3, generator=g) * 55.0).clamp(0, 255).to(torch.uint8).numpy()
