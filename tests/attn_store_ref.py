"""Reference, inputs, metric and case matrix of the token-map store kernels (csrc/attn_store.hip), shared by the CPU test of the
reference (tests/test_attn_store_ref.py) and the GPU matrix (tests/test_attn_store_kernels_gpu.py).

The store reads bf16 operands - Q pre-scaled by d^-1/2 log2 e, head h at column h*DP, zero padded from d to DP - and all of its arithmetic
behind the bf16 products is fp32.  `probs_avg_ref` takes exactly those operands and does the same computation in fp64; `probs_avg_fp32`
is the control: the same computation in torch fp32, which says how far an honest fp32 implementation lands from the fp64 one."""
import functools
import math

import torch

A_BAR = 2.0 ** -23          # absolute term of the bar: one fp32 ulp of a probability near 1 (exp2 flushing to zero, rounding of the head sum)
A_CONTROL = 1e-7            # absolute term at which the control's R is taken
B5, B6, B17, B18 = 1 << 5, 1 << 6, 1 << 17, 1 << 18      # rt_op_gemm_debug: two-pass kernel | no statistics pair | own statistics | apply v1


def dp_of(d):
    return 32 if d <= 32 else 64 if d <= 64 else 96 if d <= 96 else 160


def pack_heads(t, H, d, DP, scale=1.0):
    """fp32 [rows, H, d] -> bf16 [rows, H*DP], zero padded (the layout of AttnArgs / AttnStoreArgs)"""
    out = torch.zeros(t.shape[0], H, DP)
    out[:, :, :d] = t * scale
    return out.reshape(t.shape[0], H * DP).to(torch.bfloat16)


def q_scale(d):
    return d ** -0.5 * math.log2(math.e)


def make_qk(H, N, NK, NKrows, d, family, seed, self_attn=False):
    """q [N, H, d], k [NKrows, H, d] fp32.  family "plain": N(0,1); "spiked": a dominant key column, one key = 8 q of one query in the last
    valid key, every score ~290 below zero in the log2 domain (q[d-1] = 40, k[d-1] = -40) and ~290 above for one mirrored query.
    Key rows behind NK hold 50 N(0,1): the "anything finite" of the contract."""
    g = torch.Generator().manual_seed(seed)
    q = torch.randn(N, H, d, generator=g)
    k = torch.randn(NKrows, H, d, generator=g)
    if family == "spiked":
        k[5] *= 6.0
        k[NK - 1] = 8.0 * q[N // 3]
        q[..., d - 1] = 40.0
        k[..., d - 1] = -40.0
        q[(2 * N) // 3, :, d - 1] = -40.0
    else:
        assert family == "plain"
    if NKrows > NK:
        k[NK:] = 50.0 * torch.randn(NKrows - NK, H, d, generator=g)
    assert not self_attn or N == NK == NKrows
    return q, k


def _scores(Q, K, H, DP, NK, dtype):
    N = Q.shape[0]
    q = Q.to(dtype).reshape(N, H, DP).permute(1, 0, 2)
    k = K[:NK].to(dtype).reshape(NK, H, DP).permute(1, 0, 2)
    return torch.bmm(q, k.transpose(1, 2))                       # [H, N, NK], log2 domain


def probs_avg_ref(Q, K, H, d, DP, NK, head0=False, drop_last=False):
    """fp64: mean over heads of 2^(s - max) / sum over the first NK keys.  Q [N, H*DP], K [>= NK, H*DP] bf16 as the kernel reads them
    (d only documents the packing: columns d..DP-1 are zero).  head0 / drop_last: the two deliberately wrong variants of the
    discrimination control (head 0 instead of the head average; key NK - 1 left out of the softmax and reported as 0)."""
    assert Q.dtype == torch.bfloat16 and K.dtype == torch.bfloat16 and Q.shape[1] == H * DP and d <= DP
    s = _scores(Q, K, H, DP, NK, torch.float64)
    if drop_last:
        s[..., NK - 1] = -float("inf")
    p = torch.exp2(s - s.max(-1, True)[0])
    p = p / p.sum(-1, True)
    return p[0] if head0 else p.mean(0)


def probs_avg_fp32(Q, K, H, d, DP, NK):
    """The control: the same computation in torch fp32 on the CPU."""
    s = _scores(Q, K, H, DP, NK, torch.float32)
    p = torch.exp2(s - s.max(-1, True)[0])
    p = p / p.sum(-1, True)
    return p.mean(0)


def max_abs_score(Q, K, H, DP, NK):
    return _scores(Q, K, H, DP, NK, torch.float64).abs().max().item()


def needed_R(got, ref, A):
    """smallest R with |got - ref| <= A + R ref everywhere (ref: fp64 probabilities, >= 0)"""
    err = (got.double() - ref).abs() - A
    bad = err > 0
    if not bad.any():
        return 0.0
    return (err[bad] / ref[bad].clamp_min(1e-300)).max().item()


def rel_l2(got, ref):
    return ((got.double() - ref).pow(2).sum() / ref.pow(2).sum()).sqrt().item()


def bar_R(R_control, NKpad):
    """16 R_control + NKpad 2^-23: the control's own distance, times 16 for the kernels' other summation order (16-key MFMA tiles, eight
    waves, heads over four waves) and the 1-ulp hardware exp2, plus the worst case of an fp32 row sum of NKpad terms in any order
    ((n - 1) 2^-24), doubled for the rounding of the fp32 score accumulation."""
    return 16.0 * R_control + NKpad * 2.0 ** -23


def control_bound(smax, NK):
    """What an honest fp32 evaluation may need as R at A_CONTROL, from the format alone: the score passes through about eight fp32
    roundings (products accumulated in fp32, the subtraction of the row maximum), each at most half an ulp of the largest |s|, and a
    perturbation ds of a log2-domain score changes its probability by the factor 2^ds; the row sum of NK terms adds (NK - 1) 2^-24."""
    return 8.0 * 2.0 ** -24 * max(1.0, smax) + NK * 2.0 ** -24


# (H, N, NK, NKpad, NKrows, d, ((route name, debug bits), ...)); the first route is the one launch_attn_store takes by default
STORE_CASES = [
    # one-pass attn_store16_kernel, DP 160 / 96 / 64 / 32
    (8, 72, 77, 96, 96, 160, (("store16", 0), ("chunked", B5))),
    (8, 264, 77, 96, 96, 80, (("store16", 0), ("chunked", B5))),
    (5, 80, 77, 96, 96, 40, (("store16", 0),)),
    (4, 48, 154, 192, 192, 32, (("store16", 0), ("chunked", B5))),
    (3, 200, 200, 224, 200, 80, (("store16", 0),)),
    (2, 32, 1024, 1024, 1024, 160, (("store16", 0),)),           # all eight tiles of all eight waves, at the head dim the statistics pair refuses
    (2, 40, 231, 288, 288, 64, (("store16", B6), ("stats+apply2", 0))),      # a three-window prompt: the engine passes no scratch, i.e. bit 6's route
    # statistics + apply
    (3, 328, 328, 352, 328, 80, (("stats+apply", 0), ("chunked", B5))),
    (8, 1024, 1024, 1024, 1024, 80, (("stats+apply", 0),)),     # SD-v1.5's own 32x32 map
    (1, 256, 256, 256, 256, 32, (("stats+apply", 0),)),
    (6, 400, 400, 416, 400, 8, (("stats+apply", 0),)),
    (5, 272, 272, 288, 272, 40, (("stats+apply2", 0), ("stats+apply64", B18))),
    (20, 1024, 1024, 1024, 1024, 64, (("stats+apply2", 0), ("stats+apply64", B18))),      # SDXL's map
    # chunked attn_store_kernel
    (2, 40, 1300, 1312, 1300, 64, (("chunked", 0),)),
    (10, 64, 4096, 4096, 4096, 64, (("chunked", 0),)),
]
FAMILIES = ("plain", "spiked")
# hand-over (rt_op_attention_store_handover): self-attention (H, N, d) and cross-attention (H, N) at 77 keys, d = 64
HANDOVER_SELF = [(3, 328, 80), (8, 1024, 80), (1, 256, 32), (5, 272, 40), (20, 1024, 64)]
HANDOVER_CROSS = [(2, 64), (10, 192), (20, 128)]
HANDOVER_B = 3


def case_seed(*key):
    return sum((i + 1) * 7919 * int(v) for i, v in enumerate(key)) % (2 ** 31)


@functools.lru_cache(maxsize=4)
def reference(Q_key, H, d, DP, NK, NKpad, variants=False):
    """(ref fp64 [N, NK], R_control, bar R) of the operands registered under Q_key by `register`; with `variants` also the two wrong references."""
    Q, K = _operands[Q_key]
    ref = probs_avg_ref(Q, K, H, d, DP, NK)
    Rc = needed_R(probs_avg_fp32(Q, K, H, d, DP, NK), ref, A_CONTROL)
    out = (ref, Rc, bar_R(Rc, NKpad))
    if variants:
        out += (probs_avg_ref(Q, K, H, d, DP, NK, head0=True), probs_avg_ref(Q, K, H, d, DP, NK, drop_last=True))
    return out


_operands = {}


def register(key, Q, K):
    """The CPU bf16 operands of a case, kept unchanged for every test that shares its reference."""
    if key not in _operands:
        if len(_operands) > 8:
            _operands.clear(); reference.cache_clear()
        _operands[key] = (Q, K)
    return key


def store_operands(H, N, NK, NKpad, NKrows, d, family):
    """bf16 CPU operands of one store case: Q [N, H*DP], K [NKrows, H*DP]"""
    key = ("store", H, N, NK, NKrows, d, family)
    if key not in _operands:
        DP = dp_of(d)
        q, k = make_qk(H, N, NK, NKrows, d, family, case_seed(H, N, NK, d, FAMILIES.index(family)))
        register(key, pack_heads(q, H, d, DP, q_scale(d)), pack_heads(k, H, d, DP))
    return key, _operands[key]
