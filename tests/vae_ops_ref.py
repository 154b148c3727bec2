"""fp64 references, input builders, fault emulations and bars of the VAE's kernels, one kernel at a time (csrc/vae_kernels.hip, the
hi / lo contraction routes of csrc/gemm.hip / gemm16.hip, GroupNorm forward with low planes: csrc/norm.hip).  Shared by the CPU test of
the references (tests/test_vae_ops_ref.py) and the GPU tests (tests/test_vae_ops_gpu.py).  Plain torch: every function runs on a CPU
tensor and on the GPU alike.

A value v travels through the precise VAE as the bf16 PAIR hi = bf16(v), lo = bf16(v - hi) (16 mantissa bits).  Every reference here
reads exactly the operands the kernel reads - the rounded planes - and evaluates the operator in fp64, so what is left is the kernel's
own arithmetic (fp32 accumulation, __expf, fp32 reductions).

Metrics.  Contraction: E = max|err| / rms(ref).  Everything else: the smallest R with |err| <= rel |ref| + R (rms(ref) + |ref|) for
every element (needed_R) - hiputil.report's atol + rtol |ref| with atol = R rms(ref), rtol = R - where `rel` is the DERIVED part: 2^-8
for a bf16 hi plane alone, 2^-16 for hi + lo, 0 for fp32 outputs.

Bars.  Derived ones are stated where they are used (bit equality, 2^-22 / 2^-21 sum bounds, the 2^-8 / 2^-16 of a plane / pair, which
round-to-nearest attains: 1 + 2^-8 rounds to 1).  The others are 8 x the largest error of the shipped kernels against these references
over all cases of tests/test_vae_ops_gpu.py on an MI355X (4 x input dependence, 2 x compiler and clock variation); the measured numbers
stand in MEASURED below and, per case, in profiles/vae_ops_parity.txt.  tests/test_vae_ops_ref.py proves on the CPU, for the inputs the
GPU tests use, that every emulated fault exceeds its bar by at least 10 x and that an fp32 evaluation of the same formula stays under it.
"""
import math

import torch
import torch.nn.functional as F

# ------------------------------------------------------------------------------------------------------------------- measured bars
# name: largest error of the shipped kernels against the references below, over every case of tests/test_vae_ops_gpu.py, on an MI355X
# (profiles/vae_ops_parity.txt holds the per-case figures).  Units: E for the contraction, R elsewhere - for the outputs that exist as bf16
# planes only, R is what is left BEYOND the rounding of the planes themselves (rel = 2^-8 / 2^-16, which RNE attains), so it is tiny or 0.
# bar = 8 x max(measured, 2^-23): 4 x for input dependence, 2 x for compiler and clock variation; no fp32 kernel is held to less than
# 8 ulp of fp32 (a measured 0 says that no element sat at the rounding bound of its plane, not that the arithmetic is exact).
EPS32 = 2.0 ** -23
MEASURED = {
    "contraction": 4.2638e-06,              # hi / lo contraction, every route, against T3 (PATCH-conv3-32x56x64to136); bar 3.41e-5 <= CONTRACTION_CEILING
    "gn_fwd": 4.9052e-08,                   # GroupNorm forward planes against fp64 (C512-G32-HW200)
    "gn_stats": 1.2030e-07,                 # its (mean, rstd) (C96-G8-HW50-B2)
    "gn_bwd": 1.0616e-06,                   # GroupNorm backward, statistics as the forward entry left them (C64-G8-HW2304, fp32 out)
    "gn_bwd_exact": 1.0616e-06,             # ... with fp64 statistics rounded to fp32
    "softmax": 0.0,                         # planes against the fp64 softmax
    "softmax_bwd": 1.3934e-07,              # (4 x 400, pair)
    "color_grad": 5.1062e-08,               # (n = 16, pair)
    "color_loss": 1.3172e-07,               # relative error of the loss (n = 1)
}
SINGLE_PASS_MEASURED = 2.0123e-06           # A_lo == NULL against hi.hi in fp64, E (PATCH-conv3-32x56x64to136): asserted at the F32_OUT bar of the existing GEMM tests
CONTRACTION_CEILING = 4e-4                  # one tenth of the smallest single-pass fault (4.4e-3): the contraction bar may never exceed it
HI_REL, PAIR_REL = 2.0 ** -8, 2.0 ** -16


def bar(name):
    return 8.0 * max(MEASURED[name], EPS32)


# ------------------------------------------------------------------------------------------------------------------- pairs and metrics
def gen(seed):
    return torch.Generator().manual_seed(seed)


def split(x):
    """fp32 -> (hi, lo) bf16 planes: hi = bf16(x), lo = bf16(x - hi) (x - hi is exact in fp32)."""
    x = x.float()
    hi = x.to(torch.bfloat16)
    return hi, (x - hi.float()).to(torch.bfloat16)


def pair64(hi, lo=None):
    return hi.double() if lo is None else hi.double() + lo.double()


def rms(t):
    return t.double().pow(2).mean().sqrt().item()


def max_over_rms(got, ref):
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    return (got - ref).abs().max().item() / rms(ref)


def needed_R(got, ref, rel=0.0):
    """smallest R with |got - ref| <= rel |ref| + R (rms(ref) + |ref|) everywhere (inf when got is not finite)."""
    got, ref = got.double(), ref.double()
    if not bool(torch.isfinite(got).all()):
        return math.inf
    err = ((got - ref).abs() - rel * ref.abs()).clamp_min(0.0)
    return (err / (rms(ref) + ref.abs())).max().item()


def rel_l2(got, ref):
    got, ref = got.double(), ref.double()
    return ((got - ref).pow(2).sum() / ref.pow(2).sum()).sqrt().item()


# ------------------------------------------------------------------------------------------------------------------- hi / lo contraction
def im2col(x, mode, Ho, Wo):
    """[H, W, C] -> [Ho Wo, 9 C] (tap-major, ky outer), any float type.  mode 1: stride 1, padding 1 | 3: behind a nearest-2x up-sample |
    4: stride 2, zero padding on the bottom / right only (diffusers Downsample2D(padding=0))."""
    if mode == 3:
        x = x.repeat_interleave(2, dim=0).repeat_interleave(2, dim=1)
    H, W, Cc = x.shape
    if mode == 4:
        xp = torch.zeros(H + 1, W + 1, Cc, dtype=x.dtype, device=x.device)
        xp[:H, :W] = x
        st = 2
    else:
        xp = torch.zeros(H + 2, W + 2, Cc, dtype=x.dtype, device=x.device)
        xp[1:H + 1, 1:W + 1] = x
        st = 1
    taps = [xp[ky:ky + st * (Ho - 1) + 1:st, kx:kx + st * (Wo - 1) + 1:st] for ky in range(3) for kx in range(3)]
    return torch.cat(taps, dim=-1).reshape(Ho * Wo, 9 * Cc)


def hilo_shape(c):
    """(M, N, K, Ho, Wo) of a tests/memcases.py HILO case."""
    if c["mode"] == 0:
        return c["M"], c["N"], c["K"], 0, 0
    Ho, Wo = {1: (c["H"], c["W"]), 3: (2 * c["H"], 2 * c["W"]), 4: (c["H"] // 2, c["W"] // 2)}[c["mode"]]
    return Ho * Wo, c["Cout"], 9 * c["Cin"], Ho, Wo


def hilo_inputs(c, seed=11):
    """The operands of a HILO case on the CPU: A (dense [M, K] / image [H, W, Cin]) and W [N, K] as (hi, lo) pairs of N(0, 1) / N(0, 1/K)
    values (products of rms 1), bias [N] / res [M, N] fp32 N(0, 1/16) or None - small beside the product, so that a fault of the
    product is not diluted in rms(ref) (a lost bias or residual is still an error of order 1/4)."""
    M, N, K, _, _ = hilo_shape(c)
    g = gen(seed)
    a = torch.randn(M, K, generator=g) if c["mode"] == 0 else torch.randn(c["H"], c["W"], c["Cin"], generator=g)
    w = torch.randn(N, K, generator=g) * K ** -0.5
    bias = 0.25 * torch.randn(N, generator=g) if c["bias"] else None
    res = 0.25 * torch.randn(M, N, generator=g) if c["res"] else None
    return split(a), split(w), bias, res


def t3(c, A, W, bias, res, single=False, fault=None, dtype=torch.float64):
    """T3 = hi.hi + lo.hi + hi.lo (+ bias + res) of the planes A = (hi, lo), W = (hi, lo) in `dtype` (fp64: the reference; fp32: the
    fp32-accumulated control).  single: A_lo == NULL, hi.hi only.  fault: one of HILO_FAULTS."""
    M, N, K, Ho, Wo = hilo_shape(c)

    def mat(p):
        p = p.to(dtype)
        return p if c["mode"] == 0 else im2col(p, c["mode"], Ho, Wo)
    ah, al, wh, wl = mat(A[0]), mat(A[1]), W[0].to(dtype), W[1].to(dtype)
    hh, lh, hl = ah @ wh.t(), al @ wh.t(), ah @ wl.t()
    add = torch.zeros(M, N, dtype=dtype, device=hh.device)
    if bias is not None:
        add = add + bias.to(dtype)
    if res is not None:
        add = add + res.to(dtype)
    if single:
        assert fault is None
        return hh + add
    if fault is None:
        return hh + lh + hl + add
    if fault == "drop_lo_hi":
        return hh + hl + add
    if fault == "drop_hi_lo":
        return hh + lh + add
    if fault == "double_lo_hi":
        return hh + 2 * lh + hl + add
    if fault == "double_hi_lo":
        return hh + lh + 2 * hl + add
    if fault == "lo_of_wrong_operand":                   # the second pass multiplies A_lo with W_lo instead of W
        return hh + al @ wl.t() + hl + add
    if fault == "bias_every_pass":
        return hh + lh + hl + add + (2 * bias.to(dtype) if bias is not None else 0)
    if fault == "res_every_pass":
        return hh + lh + hl + add + (2 * res.to(dtype) if res is not None else 0)
    if fault == "a_lo_k_tail":
        # the A_lo pass reads its K tail (K up to the next multiple of the 64-wide K tile) from memory instead of the zero page: the
        # contract run of the GPU test has NaN there (padded lda, poisoned) and W's tail is the zero page: NaN x 0
        if c["mode"] != 0 or K % 64 == 0:
            return hh + lh + hl + add
        return hh + lh + hl + add + float("nan") * 0.0
    raise ValueError(fault)


HILO_FAULTS = ("drop_lo_hi", "drop_hi_lo", "double_lo_hi", "double_hi_lo", "lo_of_wrong_operand", "bias_every_pass", "res_every_pass", "a_lo_k_tail")


def hilo_fault_applies(c, fault):
    M, N, K, _, _ = hilo_shape(c)
    return {"bias_every_pass": c["bias"], "res_every_pass": bool(c["res"]), "a_lo_k_tail": c["mode"] == 0 and K % 64 != 0}.get(fault, True)


# ------------------------------------------------------------------------------------------------------------------- rt_op_split_bf16
SPLIT_SIZES = (3 * 1024 - 4, 3 * 1024 + 4, 2048 * 1024 + 4)      # grid of one partial block / ragged / past the 2048-block cap (second grid-stride trip)


def split_values(n, seed=5):
    """N(0, 1) values with the edge cases up front: +-0, 1e+-30, and values whose residual is exactly representable in bf16 (1 + 2^-9:
    hi = 1, lo = 2^-9; 3 + 2^-7 + 2^-14)."""
    x = torch.randn(n, generator=gen(seed))
    edge = torch.tensor([0.0, -0.0, 1e30, -1e30, 1e-30, -1e-30, 1.0 + 2.0 ** -9, -(1.0 + 2.0 ** -9), 3.0 + 2.0 ** -7 + 2.0 ** -14, 0.5 - 2.0 ** -11,
                         65280.0, 2.0 ** -100])
    x[:edge.numel()] = edge
    x[-2:] = torch.tensor([1.0 + 2.0 ** -9, -1e30])
    return x


# ------------------------------------------------------------------------------------------------------------------- GroupNorm
# (C, G, HW, B): 64 ch | a float4 = one group | last chunk of 8 rows, clamped unroll rows | idle row lanes (256 % 24 != 0) + a 2-row chunk,
# B = 2 | nv = 320 >= 256: the second `vec += 256` trip | 18-row chunks, two-launch forward
GN_CASES = [(64, 8, 144, 1), (128, 32, 400, 1), (512, 32, 200, 1), (96, 8, 50, 2), (1280, 32, 48, 1), (64, 8, 2304, 1)]
GN_EPS = 1e-6
# crossed over the cases (not a full product): x bf16, dA_lo, silu, add, out (fp32), out_bf16_lo
GN_VARIANTS = [dict(x_bf16=False, da_lo=True, silu=True, add=True, out=True, out_lo=True),
               dict(x_bf16=True, da_lo=False, silu=True, add=False, out=False, out_lo=False),
               dict(x_bf16=False, da_lo=True, silu=False, add=True, out=True, out_lo=True),
               dict(x_bf16=False, da_lo=False, silu=True, add=False, out=True, out_lo=False),
               dict(x_bf16=True, da_lo=True, silu=False, add=True, out=False, out_lo=True),
               dict(x_bf16=False, da_lo=True, silu=True, add=False, out=True, out_lo=True)]


def gn_id(case, v):
    return "C%d-G%d-HW%d-B%d-" % case + "-".join(k for k, on in v.items() if on)


def gn_stats(x64, G):
    """(mean, rstd) [B, G] of x [B, HW, C] in x's precision."""
    B, HW, Cc = x64.shape
    xg = x64.reshape(B, HW, G, Cc // G)
    mean = xg.mean(dim=(1, 3))
    var = (xg - mean[:, None, :, None]).pow(2).mean(dim=(1, 3))
    return mean, (var + GN_EPS).rsqrt()


def _per_channel(s, Cc):
    """[B, G] -> [B, 1, C]"""
    return s.repeat_interleave(Cc // s.shape[1], dim=1)[:, None, :]


def gn_inputs(case, v, seed=21):
    """x [B, HW, C] (fp32, or bf16-representable), gamma / beta [C], dA = randn + 0.75 + 0.75 xh as a pair (lo dropped without da_lo),
    add [B, HW, C] or None.  Channels differ in scale and offset, so groups differ in mean and variance."""
    Cc, G, HW, B = case
    g = gen(seed + Cc + HW)
    x = torch.randn(B, HW, Cc, generator=g) * (0.5 + torch.rand(Cc, generator=g)) + (2 * torch.rand(Cc, generator=g) - 1)
    if v["x_bf16"]:
        x = x.to(torch.bfloat16).float()
    gamma = 0.5 + torch.rand(Cc, generator=g)
    beta = 0.5 * torch.randn(Cc, generator=g)
    mean, rstd = gn_stats(x.double(), G)
    xh = ((x.double() - _per_channel(mean, Cc)) * _per_channel(rstd, Cc)).float()
    dA = split(torch.randn(B, HW, Cc, generator=g) + 0.75 + 0.75 * xh)
    if not v["da_lo"]:
        dA = (dA[0], None)
    add = torch.randn(B, HW, Cc, generator=g) if v["add"] else None
    return x, gamma, beta, dA, add


def _silu_or_id(y, silu):
    return y * torch.sigmoid(y) if silu else y


def gn_fwd_ref(x, G, gamma, beta, silu):
    """fp64: (GroupNorm(x) (+ SiLU), mean, rstd)"""
    x = x.double()
    Cc = x.shape[2]
    mean, rstd = gn_stats(x, G)
    y = (x - _per_channel(mean, Cc)) * _per_channel(rstd, Cc) * gamma.double() + beta.double()
    return _silu_or_id(y, silu), mean, rstd


def gn_bwd_ref(x, dA, G, gamma, beta, silu, add):
    """d/dx of sum(act(GroupNorm(x)) o dA) by autograd in fp64 (+ add): the backward of the whole operator, statistics included."""
    x = x.double().clone().requires_grad_(True)
    Cc = x.shape[2]
    y = F.group_norm(x.transpose(1, 2), G, gamma.double(), beta.double(), GN_EPS).transpose(1, 2)
    (_silu_or_id(y, silu) * dA.double()).sum().backward()
    return x.grad + (add.double() if add is not None else 0.0)


def gn_bwd_formula(x, dA, mean, rstd, G, gamma, beta, silu, add, fault=None, dtype=torch.float64):
    """csrc/common.h: dx = rstd (dxh - mean_g(dxh) - xh mean_g(dxh xh)), dxh = dA silu'(y) gamma, y = xh gamma + beta, from GIVEN
    statistics [B, G].  fault: one of GN_BWD_FAULTS."""
    x, dA, mean, rstd, gamma, beta = (t.to(dtype) for t in (x, dA, mean, rstd, gamma, beta))
    B, HW, Cc = x.shape
    if fault == "wrong_group_stats":
        mean, rstd = mean.roll(1, dims=1), rstd.roll(1, dims=1)
    mu, rs = _per_channel(mean, Cc), _per_channel(rstd, Cc)
    xh = (x - mu) * rs
    dy = dA
    if silu:
        y = xh * gamma + beta
        sg = torch.sigmoid(y)
        dy = dy * (sg if fault == "sigmoid_only" else sg * (1 + y * (1 - sg)))
    dxh = dy * gamma

    def gmean(t):
        return _per_channel(t.reshape(B, HW, G, Cc // G).mean(dim=(1, 3)), Cc)
    m1 = 0.0 if fault == "drop_mean_dxh" else gmean(dxh)
    m2 = 0.0 if fault == "drop_mean_dxh_xh" else gmean(dxh * xh)
    out = rs * (dxh - m1 - xh * m2)
    return out + (add.to(dtype) if add is not None else 0.0)


GN_BWD_FAULTS = ("drop_mean_dxh", "drop_mean_dxh_xh", "sigmoid_only", "wrong_group_stats")


# ------------------------------------------------------------------------------------------------------------------- softmax
SOFTMAX_CASES = [(5, 77), (3, 256), (4, 400), (2, 1024)]           # < 256 columns | exactly one trip | ragged second trip | four trips
SOFTMAX_SCALE = 64 ** -0.5


def softmax_scores(rows, cols, seed=31):
    """scores of order 8 / scale; row 0 offset by +60 / scale, row 1 by -60 / scale, the last row spiked (one score 40 / scale above the rest); the
    last column of the other rows carries e^4 times its share."""
    s = torch.randn(rows, cols, generator=gen(seed + cols)) * (2.0 / SOFTMAX_SCALE)
    s[0] += 60.0 / SOFTMAX_SCALE
    s[1] -= 60.0 / SOFTMAX_SCALE
    s[rows - 1, cols // 3] += 40.0 / SOFTMAX_SCALE
    s[:rows - 1, -1] += 4.0 / SOFTMAX_SCALE                          # a heavy last column: a strided loop that stops short is an error of percents
    return s


def softmax_ref(s):
    return torch.softmax(s.double() * SOFTMAX_SCALE, dim=-1)


def softmax_bwd_inputs(rows, cols, with_lo, seed=37):
    """P = softmax of diffuse scores as a pair (lo dropped without with_lo), dP = randn + a per-row constant of order 1."""
    g = gen(seed + cols)
    p = torch.softmax(torch.randn(rows, cols, generator=g), dim=-1)
    P = split(p)
    if not with_lo:
        P = (P[0], None)
    dp = torch.randn(rows, cols, generator=g) + (1.0 + torch.rand(rows, 1, generator=g)) * (1 - 2 * (torch.arange(rows)[:, None] % 2))
    return P, dp


def softmax_bwd_ref(P, dp, fault=None, dtype=torch.float64):
    """dS = scale P o (dP - rowsum(dP o P)), P = hi + lo as given."""
    p = P[0].to(dtype) + (P[1].to(dtype) if P[1] is not None else 0.0)
    dp = dp.to(dtype)
    dot = 0.0 if fault == "drop_dot" else (p * dp).sum(-1, keepdim=True)
    if fault == "dot_of_hi_only":
        dot = (P[0].to(dtype) * dp).sum(-1, keepdim=True)
    return SOFTMAX_SCALE * p * (dp - dot)


SOFTMAX_BWD_FAULTS = ("drop_dot",)                     # + "dot_of_hi_only" where P comes as a pair

# ------------------------------------------------------------------------------------------------------------------- transpose, sum-pool
TRANSPOSE_CASES = [(64, 64), (240, 64), (77, 200), (1, 130)]
SUMPOOL_CASES = [(1, 8, 12, 64), (2, 5, 7, 8), (1, 128, 130, 256)]      # the last: 1 064 960 float4 outputs > 4096 x 256: the grid-stride second trip


def sumpool_ref(x):
    """[B, 2H, 2W, C] -> ([B, H, W, C] sums in fp64, sum of |terms|)"""
    x = x.double()
    B, H2, W2, Cc = x.shape
    t = x.reshape(B, H2 // 2, 2, W2 // 2, 2, Cc)
    return t.sum(dim=(2, 4)), t.abs().sum(dim=(2, 4))


# ------------------------------------------------------------------------------------------------------------------- post_quant_conv
PQ_HW = (50, 256, 300)


def pq_inputs(HW, seed=41):
    g = gen(seed + HW)
    lat, eps = torch.randn(4, HW, generator=g), torch.randn(4, HW, generator=g)
    W, b = torch.randn(4, 4, generator=g) * 0.5, torch.randn(4, generator=g)
    return lat, eps, W, b, 1.0 / (0.6 * 0.18215), -0.8 / (0.6 * 0.18215)


def pq_fwd_ref(lat, eps, c_lat, c_eps, W, b, dtype=torch.float64):
    """([HW, 4] out = W z + b, z = c_lat lat + c_eps eps; sum of |terms| per output)"""
    lat, W, b = lat.to(dtype), W.to(dtype), b.to(dtype)
    t_lat = c_lat * lat
    t_eps = c_eps * eps.to(dtype) if eps is not None else torch.zeros_like(lat)
    z = t_lat + t_eps
    out = (W @ z).t() + b
    terms = (W.abs() @ (t_lat.abs() + t_eps.abs())).t() + b.abs()
    return out, terms


def pq_bwd_ref(dz, W, gscale, weight, mask_all, lat, dtype=torch.float64, fault=None):
    """dz [HW, >= 4] -> (g [4, HW] = gscale W^T dz, lat - g weight mask_all, sum of |terms| of g, ... of the update)"""
    d = dz[:, :4].to(dtype)
    W = W.to(dtype)
    Wt = W if fault == "w_not_transposed" else W.t()
    g = gscale * (Wt @ d.t())
    tg = abs(gscale) * (Wt.abs() @ d.abs().t())
    upd = g * weight * mask_all.to(dtype)
    new = lat.to(dtype) - upd
    return g, new, tg, lat.to(dtype).abs() + tg * abs(weight) * mask_all.to(dtype).abs()


# ------------------------------------------------------------------------------------------------------------------- colour loss
COLOR_HWI, COLOR_LDI, COLOR_N = 1283, 4, (1, 3, 16)


def color_inputs(n, seed=51):
    """img [HWi, 3] on the dyadic grid 2^-10 Z within [-1.5, 1.5] - with exactly +-1 and their grid neighbours on either side up front - so
    v = img / 2 + 0.5 and the clamp decision on [0, 1] are exact in fp32 and fp64 alike; masks [n, HWi]: k % 3 == 0 soft (0, 1),
    1 binary with zeros, 2 on a handful of pixels; target [n, 3] in (0, 1)."""
    g = gen(seed + n)
    img = torch.randint(-1536, 1537, (COLOR_HWI, 3), generator=g).float() / 1024.0
    q = 2.0 ** -10
    edge = torch.tensor([1.0, -1.0, 1.0 + q, -1.0 - q, 1.0 - q, -1.0 + q, 1.5, -1.5, 0.0])
    for ch in range(3):
        img[ch * 16:ch * 16 + edge.numel(), ch] = edge
        img[300 + ch, :] = torch.tensor([1.0, -1.0, 1.0 + q]).roll(ch)
    masks = torch.zeros(n, COLOR_HWI)
    for k in range(n):
        if k % 3 == 0:
            masks[k] = torch.rand(COLOR_HWI, generator=g)
        elif k % 3 == 1:
            masks[k] = (torch.rand(COLOR_HWI, generator=g) < 0.4).float()
        else:
            masks[k, torch.randperm(COLOR_HWI, generator=g)[:7]] = 1.0
        masks[k, :48:5] = 1.0 if k % 3 else 0.75                      # every mask sees some of the edge pixels
    target = torch.rand(n, 3, generator=g)
    return img, masks, target


def color_ref(img, masks, target, fault=None, dtype=torch.float64):
    """(loss, dimg [HWi, 3]) of L = sum_k 100 mean_c (avg_kc - target_kc)^2, avg = sum(clamp(img / 2 + 0.5, 0, 1) m_k) / sum(m_k);
    the clamp passes the gradient on the CLOSED interval [0, 1] (torch.clamp)."""
    img, masks, target = img.to(dtype), masks.to(dtype), target.to(dtype)
    v = img * 0.5 + 0.5
    c = v if fault == "no_clamp_in_sums" else v.clamp(0.0, 1.0)
    msum = masks.sum(-1, keepdim=True)                                  # [n, 1]
    avg = (masks @ c) / msum                                            # [n, 3]
    d = avg - target
    loss = (100.0 / 3.0) * d.pow(2).sum()
    coef = (200.0 / 3.0) * d / msum                                     # dL / d(sum_k) per region and channel
    gfull = 0.5 * (masks.t() @ coef)                                    # [HWi, 3]
    if fault == "open_interval":
        passes = (v > 0) & (v < 1)
    elif fault == "no_clamp_in_grad":
        passes = torch.ones_like(v, dtype=torch.bool)
    else:
        passes = (v >= 0) & (v <= 1)
    return loss, torch.where(passes, gfull, torch.zeros_like(gfull))


COLOR_FAULTS = ("open_interval", "no_clamp_in_grad", "no_clamp_in_sums")
