"""References for regional LoRA on ff.net.0.proj (csrc/lora.hip: lora_geglu_kernel, include/rtdiff.h: rt_op_lora_geglu) and for the wider
target set (targets="transformer": ff.net.0.proj, ff.net.2, proj_in, proj_out).  Test infrastructure, plain torch; the pieces shared with
the attention projections come from tests/regional_lora_ref.py unchanged.

  GEGLU_CASES / geglu_inputs   the shapes of the op tests and their inputs: X bf16, Z fp32 pre-activations in the packed column order (per 64
                               columns [32 value | 32 gate]; the gate columns are drawn with standard deviation 3, so they lie on both
                               sides of the polynomial's clamp at +-4.25), `up` in the packed row order and in nn.Linear's
  geglu_ref                    the fp64 restatement with the per-element bar
  emulate_geglu                a CPU emulation of an honest kernel and of seven faulty ones
  wide_modules / full_adapters synthetic adapters on all twelve module kinds of the tiny UNets, and the same files cut down to attention

THE BAR, per output element (m, c) of an adapted stream, on the exact value ref = v gelu(g), v = Zv + Dv, g = Zg + Dg, D = (f T) B^T:
    dv, dg = sum_j half_ulp_bf16(f_j T[m, j]) |B[n, j]|          ONE bf16 rounding of every Ts[m, j], propagated through |B| (n = the value /
           + GEGLU_ACC_UNITS 2^-24 S[m, n]                       gate column of c), plus the fp32 accumulation allowance on
                                                                 S = |Z| + sum_j |f_j| (sum_k |X| |A|) |B|, as tests/regional_lora_ref.py
    rest   = |gelu(g)| dv + |v| L dg + L dv dg                   propagated through the product; L = max |gelu'| = 1.12897
           + |v| 6.4e-5                                          the polynomial's documented absolute error (csrc/common.h)
           + 2^-24 |ref|                                         the fp32 product before the rounding
    bar    = half_ulp_bf16(|ref| + rest) + rest                  ONE rounding of the output
  GEGLU_ACC_UNITS is MEASURED, not chosen: the worst error of emulate_geglu's fp32 arithmetic alone (no Ts rounding; the pre-activations
  v and g against fp64) in units of 2^-24 S over GEGLU_CASES came to 0.80 (smallest 0.80 - with K = 32 and rank 4 the one fp32 addition
  Z + D is most of S -, gaps 0.19, largest-rank 0.09; tests/test_regional_lora_ff.py::test_accumulation_allowance_is_the_measured_one
  recomputes it) and is recorded as 0.8.  The GPU
  tests take it twice, as GPU_ACC_UNITS there."""
import functools
import math

import torch

import regional_lora_ref as R
from regional_lora_ref import _half_ulp, bf, factors, pad16

GEGLU_ACC_UNITS = 0.8
GPU_GEGLU_ACC_UNITS = 2 * GEGLU_ACC_UNITS
GELU_SLOPE = 1.12897             # max |gelu'(x)| = Phi(sqrt 2) + sqrt 2 phi(sqrt 2), at x = sqrt 2
GELU_POLY_ERR = 6.4e-5           # csrc/common.h: |gelu error| of the polynomial erf form, absolute, everywhere

# name, per-stream scales of the adapters (all 0 = not adapted), rows per stream, K = C, N = 8C packed columns, raw ranks
GEGLU_CASES = (
    dict(name="smallest", scales=[[0.8]], rows=8, K=32, N=64, ranks=[4]),
    dict(name="gaps-two-adapters", scales=[[0.7, -0.4], [0, 0], [1.0, 0.5], [0, 0]], rows=24, K=320, N=2560, ranks=[16, 32]),
    dict(name="largest-rank", scales=[[1.0], [-0.6]], rows=72, K=640, N=5120, ranks=[128]),
)
GEGLU_IDS = [c["name"] for c in GEGLU_CASES]


def geglu_row_map(N):
    """packed row / column r of ff.net.0.proj <- nn.Linear's row (PACK_ROWS_GEGLU): per 64 [32 value | 32 gate], gate rows start at N / 2."""
    r = torch.arange(N)
    blk, w = r >> 6, r & 63
    return torch.where(w < 32, blk * 32 + w, N // 2 + blk * 32 + (w - 32))


def split_packed(z):
    """[..., N] packed -> (value [..., N / 2], gate [..., N / 2]) in output column order."""
    b = z.reshape(*z.shape[:-1], -1, 2, 32)
    return b[..., 0, :].reshape(*z.shape[:-1], -1), b[..., 1, :].reshape(*z.shape[:-1], -1)


def geglu_inputs(case, seed=0):
    """-> dict: X [B, rows, K] bf16, Z [B, rows, N] fp32 packed, down [R, K], up [N, R] packed rows (bf16; pad rank columns zero), up_linear
    (the same rows in nn.Linear's order: the 'un-interleaved' mutant's operand), aor [R], col [R] int32, scales [B][4], pad_cols."""
    g = torch.Generator().manual_seed(2000 + seed + 17 * case["rows"] + case["K"])
    B, rows, K, N, ranks = len(case["scales"]), case["rows"], case["K"], case["N"], case["ranks"]
    Rc = sum(pad16(r) for r in ranks)
    down, up = torch.zeros(Rc, K), torch.zeros(N, Rc)
    aor, col = torch.zeros(Rc), torch.zeros(Rc, dtype=torch.int32)
    pad_cols = torch.ones(Rc, dtype=torch.bool)
    c0 = 0
    for l, r in enumerate(ranks):
        down[c0:c0 + r] = torch.randn(r, K, generator=g) / math.sqrt(K)
        up[:, c0:c0 + r] = torch.randn(N, r, generator=g) * 2.0 / math.sqrt(r)
        aor[c0:c0 + r] = 0.75 if l == 0 else 1.0
        col[c0:c0 + pad16(r)] = l
        pad_cols[c0:c0 + r] = False
        c0 += pad16(r)
    X = bf(torch.randn(B, rows, K, generator=g))
    Z = torch.randn(B, rows, N, generator=g)
    gate = (torch.arange(N) & 63) >= 32
    Z[:, :, gate] *= 3.0
    scales = [[float(s[l]) if l < len(s) else 0.0 for l in range(4)] for s in case["scales"]]
    up = bf(up)
    return dict(X=X, Z=Z, down=bf(down), up=up[geglu_row_map(N)], up_linear=up, aor=aor, col=col, scales=scales, pad_cols=pad_cols)


def gelu64(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def geglu_ref(inp, acc_units=GEGLU_ACC_UNITS):
    """fp64 restatement -> (ref, bar), both [B, rows, N / 2]; a stream whose scales are all 0 has ref = bar = 0 (its rows are not written)."""
    X, Z, A, Bm = inp["X"].double(), inp["Z"].double(), inp["down"].double(), inp["up"].double()
    ref = torch.zeros(Z.shape[0], Z.shape[1], Z.shape[2] // 2, dtype=torch.float64)
    bar = torch.zeros_like(ref)
    for b, s4 in enumerate(inp["scales"]):
        if not any(s4):
            continue
        f = factors(inp["aor"], inp["col"], s4).double()
        Ts = (X[b] @ A.t()) * f
        v, g = split_packed(Z[b] + Ts @ Bm.t())
        S = Z[b].abs() + ((X[b].abs() @ A.abs().t()) * f.abs()) @ Bm.abs().t()
        dv, dg = split_packed(_half_ulp(Ts.abs(), 8) @ Bm.abs().t() + acc_units * 2.0 ** -24 * S)
        ref[b] = v * gelu64(g)
        rest = gelu64(g).abs() * dv + v.abs() * GELU_SLOPE * dg + GELU_SLOPE * dv * dg + v.abs() * GELU_POLY_ERR + 2.0 ** -24 * ref[b].abs()
        bar[b] = _half_ulp(ref[b].abs() + rest, 8) + rest
    return ref, bar


_GELU_COEFS = (1.203002836e-10, -1.137335648e-08, 4.748426363e-07, -1.167462415e-05, 1.911683503e-04, -2.242938848e-03, 1.971663348e-02,
               -1.328222901e-01, 7.978754640e-01)


def gelu_poly(x):
    """gelu_erf of csrc/common.h in fp32: erf(x / sqrt 2) as the odd degree-17 polynomial of clamp(x, +-4.25)."""
    xc = x.clamp(-4.25, 4.25)
    s = xc * xc
    q = torch.full_like(x, _GELU_COEFS[0])
    for c in _GELU_COEFS[1:]:
        q = q * s + c
    h = x * 0.5
    return h * (xc * q) + h


MUTANTS = ("value_gate_swapped", "term_on_value_only", "term_after_gelu", "neighbour_scale", "pad_column_as_data", "uninterleaved_up")


def emulate_geglu(inp, *, mutant=None, roundings=True, pre=False):
    """An honest kernel on the CPU -> [B, rows, N / 2] bf16 (rows of streams that are not adapted: 0): T and D accumulated in fp32 over
    32-wide contraction steps, Ts = bf16(f T), fp32 Z + D, the polynomial gelu in fp32, ONE rounding.  pre=True returns the fp32
    pre-activations (v, g) instead; roundings=False leaves Ts in fp32.  mutant: MUTANTS or 'scale_after_rounding'."""
    X, Z = inp["X"], inp["Z"]
    A, Bm, aor = inp["down"].clone(), inp["up"].clone(), inp["aor"].clone()
    if mutant == "pad_column_as_data":
        g_ = torch.Generator().manual_seed(5)
        pc = inp["pad_cols"]
        A[pc] = bf(torch.randn(int(pc.sum()), A.shape[1], generator=g_) / math.sqrt(A.shape[1]))
        Bm[:, pc] = bf(torch.randn(Bm.shape[0], int(pc.sum()), generator=g_))
        aor[pc] = 1.0
    if mutant == "uninterleaved_up":
        Bm = inp["up_linear"].clone()
    nb = len(inp["scales"])
    out = torch.zeros(Z.shape[0], Z.shape[1], Z.shape[2] // 2, dtype=torch.bfloat16)
    pres = {}

    def steps(P, Q):
        acc = torch.zeros(P.shape[0], Q.shape[0], dtype=torch.float32)
        for c0 in range(0, P.shape[1], 32):
            acc = acc + (P[:, c0:c0 + 32].double() @ Q[:, c0:c0 + 32].double().t()).float()
        return acc
    for b, s4 in enumerate(inp["scales"]):
        if not any(s4):
            continue
        f = factors(aor, inp["col"], inp["scales"][(b + 1) % nb] if mutant == "neighbour_scale" else s4)
        T = steps(X[b], A)
        Ts = bf(bf(T).float() * f) if mutant == "scale_after_rounding" else (bf(T * f) if roundings else T * f)
        dv, dg = split_packed(steps(Ts, Bm))
        zv, zg = split_packed(Z[b])
        if mutant == "value_gate_swapped":
            o = (zg + dg) * gelu_poly(zv + dv)
        elif mutant == "term_on_value_only":
            o = (zv + dv) * gelu_poly(zg)
        elif mutant == "term_after_gelu":
            o = (zv + dv) * (gelu_poly(zg) + dg)
        else:
            o = (zv + dv) * gelu_poly(zg + dg)
        pres[b] = (zv + dv, zg + dg)
        out[b] = bf(o)
    return pres if pre else out


def measured_acc_units(case):
    """The worst error of the honest emulation's fp32 arithmetic ALONE (no Ts rounding) on the pre-activations against fp64, in units of
    2^-24 S (see the module docstring)."""
    inp = geglu_inputs(case)
    X, Z, A, Bm = inp["X"].double(), inp["Z"].double(), inp["down"].double(), inp["up"].double()
    got = emulate_geglu(inp, roundings=False, pre=True)
    worst = 0.0
    for b, s4 in enumerate(inp["scales"]):
        if not any(s4):
            continue
        f = factors(inp["aor"], inp["col"], s4).double()
        ref = split_packed(Z[b] + ((X[b] @ A.t()) * f) @ Bm.t())
        S = split_packed(Z[b].abs() + ((X[b].abs() @ A.abs().t()) * f.abs()) @ Bm.abs().t())
        for k in range(2):
            worst = max(worst, ((got[b][k].double() - ref[k]).abs() / (2.0 ** -24 * S[k])).max().item())
    return worst


# ---------------------------------------------------------------------------------------------------------------- checkpoints
WIDE_LEAVES = (".ff.net.0.proj", ".ff.net.2", ".proj_in", ".proj_out")
# Gains of the two synthetic adapters of the forward tests: those of tests/test_regional_lora_gpu.py.  With them the merged oracle without
# the four further modules is 0.29 .. 0.82 (19 .. 54 forward bars) from the full one on the tiny forwards, far beyond the three bars
# tests/test_regional_lora_ff.py::test_the_forward_cases_discriminate asks for: no larger gain is needed.
GAIN_A, GAIN_B = 2.0, 1.0


def wide_modules(sd):
    """The module paths of ff.net.0.proj, ff.net.2 of every transformer block and proj_in / proj_out of every transformer, in sd's order."""
    return [k[:-7] for k in sd if k.endswith(".weight") and ".attentions." in k and k[:-7].endswith(WIDE_LEAVES)]


def attention_part(ck, sd):
    """A checkpoint cut down to its tensors on the attention projections (what a merge 'on attention modules only' merges)."""
    from rich_text_to_image_amd.lora import resolve_targets
    keep = set(R.attention_projections(sd))
    out = {}
    for key, t in ck.items():
        if next(iter(resolve_targets(sd, {key: t})[1])) in keep:
            out[key] = t
    return out


@functools.lru_cache(maxsize=None)
def full_adapters(which):
    """Two synthetic adapters on all twelve module kinds of the tiny UNet: (state dict, [checkpoint A (kohya, rank 4, alpha 2), B (peft,
    rank 8)], the same two cut down to attention)."""
    from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict
    cfg = TINY_XL_CONFIG if which == "xl" else TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=11)
    ckA, _ = R.synthetic_adapter(sd, rank=4, alpha=2.0, seed=1, layout="kohya", gain=GAIN_A, extra=wide_modules(sd))
    ckB, _ = R.synthetic_adapter(sd, rank=8, seed=2, layout="peft", gain=GAIN_B, extra=wide_modules(sd))
    return sd, [ckA, ckB], [attention_part(ckA, sd), attention_part(ckB, sd)]
