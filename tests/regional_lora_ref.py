"""References for regional LoRA (csrc/lora.hip, include/rtdiff.h: rt_op_lora_add; rich-text-to-image_amd/regional_lora.py).  Test
infrastructure, plain torch.

  OP_CASES / op_inputs    the shapes of the op tests and their inputs (bf16 values, the packed layouts: head-padded `up`, to_q's qscale)
  op_ref                  the fp64 restatement of the three lines of the kernel on those values, with the per-element bar
  emulate                 a CPU emulation of an honest kernel (bf16 operands, fp32 accumulation in 32-wide contraction steps, Ts rounded
                          to bf16 once, one rounding to the output type) and of seven faulty ones
  synthetic_adapter       a LoRA checkpoint for a UNet state dict, kohya / peft / diffusers layouts

THE OP BAR, per output element (m, n) of an adapted stream, on the exact value ref = Y + sum_j f_j T[m, j] B[n, j]:
    bar = half_ulp_out(|ref| + rest)                            ONE rounding to the output type (bf16: 8 significant bits, fp16: 11)
        + sum_j half_ulp_bf16(f_j T[m, j]) |B[n, j]|            ONE bf16 rounding of every Ts[m, j], propagated through |B|
        + ACC_UNITS 2^-24 S[m, n]                               fp32 accumulation (`rest` = the two lines above this one)
  with S = |Y| + sum_j |f_j| (sum_k |X[m, k]| |A[j, k]|) |B[n, j]|, the sum of the magnitudes of everything that is added up.
  ACC_UNITS is MEASURED, not derived: the worst error of emulate()'s fp32 arithmetic alone (the emulation without its two roundings)
  against fp64, in units of 2^-24 S, over OP_CASES came to 0.41 (smallest 0.41, gaps 0.15, largest-rank 0.06, cache 0.17, fp16 0.09;
  tests/test_regional_lora.py::test_accumulation_allowance_is_the_measured_one recomputes it) and is recorded as 0.5.  The GPU
  tests take it twice (GPU_ACC_UNITS): the MFMA's accumulation order inside a 32-wide step differs from the emulation's."""
import math

import torch

ACC_UNITS = 0.5
GPU_ACC_UNITS = 2 * ACC_UNITS

# name, streams, per-stream scales of the (up to two) adapters - all 0 = the stream is not adapted -, rows per stream, K, N, raw ranks,
# output form, (heads, d, DP) of a head-padded `up` or None, to_q (the packed `up` carries d^-1/2 log2 e)
OP_CASES = (
    dict(name="smallest", scales=[[0.8]], rows=8, K=32, N=16, ranks=[4], form="bf16", heads=None, to_q=False),
    dict(name="gaps-headpad-two-adapters", scales=[[0.7, -0.4], [0, 0], [1.0, 0.5], [0, 0]], rows=24, K=320, N=384, ranks=[16, 32], form="bf16",
         heads=(8, 40, 48), to_q=True),
    dict(name="largest-rank", scales=[[1.0], [-0.6]], rows=72, K=1280, N=1280, ranks=[128], form="bf16", heads=None, to_q=False),
    dict(name="cache-row-major", scales=[[0.9, 0.0], [0.0, 0.0], [0.3, 1.1]], rows=96, K=2048, N=640, ranks=[12, 32], form="bf16", heads=None, to_q=False),
    dict(name="cache-transposed", scales=[[0.9, 0.0], [0.0, 0.0], [0.3, 1.1]], rows=96, K=2048, N=640, ranks=[12, 32], form="bf16_t", heads=None, to_q=False),
    dict(name="fp16-trunk", scales=[[0.7], [1.2]], rows=1024, K=640, N=640, ranks=[64], form="f16", heads=None, to_q=False),
)
CASE_IDS = [c["name"] for c in OP_CASES]


def bf(x):
    return x.to(torch.bfloat16)


def pad16(r):
    return -(-r // 16) * 16


def op_inputs(case, seed=0):
    """-> dict: X [B, rows, K], Y [B, rows, N] (the output type's values), down [R, K], up [N, R] (bf16 values, packed: pad rank columns
    zero, head-pad rows zero, qscale inside `up`), aor [R] fp32, col [R] int32, scales [B][4], up_raw (bf16 values before the qscale, the
    'qscale missing' mutant's operand), pad_cols / pad_rows (bool masks)."""
    g = torch.Generator().manual_seed(1000 + seed + 17 * case["rows"] + case["K"])
    B, rows, K, N, ranks = len(case["scales"]), case["rows"], case["K"], case["N"], case["ranks"]
    R = sum(pad16(r) for r in ranks)
    down, up = torch.zeros(R, K), torch.zeros(N, R)
    aor, col = torch.zeros(R), torch.zeros(R, dtype=torch.int32)
    pad_cols = torch.ones(R, dtype=torch.bool)
    c0 = 0
    for l, r in enumerate(ranks):
        down[c0:c0 + r] = torch.randn(r, K, generator=g) / math.sqrt(K)
        up[:, c0:c0 + r] = torch.randn(N, r, generator=g) * 2.0 / math.sqrt(r)
        aor[c0:c0 + r] = (r / 2.0 if l == 0 else float(r)) / r * (1.5 if l == 0 else 1.0)          # alpha / rank: 0.75 and 1.0
        col[c0:c0 + pad16(r)] = l
        pad_cols[c0:c0 + r] = False
        c0 += pad16(r)
    pad_rows = torch.zeros(N, dtype=torch.bool)
    if case["heads"]:
        H, d, DP = case["heads"]
        assert H * DP == N
        pad_rows = (torch.arange(N) % DP) >= d
        up[pad_rows] = 0
    up_raw = bf(up)
    if case["to_q"]:
        up = up_raw.float() * (case["heads"][1] ** -0.5 * math.log2(math.e))
    X = bf(torch.randn(B, rows, K, generator=g))
    Y = torch.randn(B, rows, N, generator=g)
    Y = Y.to(torch.float16) if case["form"] == "f16" else bf(Y)
    scales = [[float(s[l]) if l < len(s) else 0.0 for l in range(4)] for s in case["scales"]]
    return dict(X=X, Y=Y, down=bf(down), up=bf(up), up_raw=up_raw, aor=aor, col=col, scales=scales, pad_cols=pad_cols, pad_rows=pad_rows)


def factors(aor, col, scale4):
    """f[j] = scale[adapter(j)] alpha_over_rank[j], as the kernel forms it: one fp32 product."""
    return (torch.tensor(scale4, dtype=torch.float32)[col.long()] * aor.float())


def _half_ulp(v, bits):
    """Half an ulp of a format with `bits` significant bits at magnitude v (fp64 tensor); fp16's subnormal floor for bits == 11."""
    e = torch.floor(torch.log2(v.clamp_min(1e-300)))
    if bits == 11:
        e = e.clamp_min(-14.0)
    return torch.where(v > 0, torch.exp2(e - bits), torch.zeros_like(v))


def op_ref(inp, form, acc_units=ACC_UNITS):
    """fp64 restatement on the given values -> (ref, bar), both [B, rows, N] (logical: the transposed form is the same numbers stored
    transposed); a stream whose scales are all 0 is Y itself with bar 0."""
    X, Y, A, Bm = inp["X"].double(), inp["Y"].double(), inp["down"].double(), inp["up"].double()
    ref, bar = Y.clone(), torch.zeros_like(Y)
    out_bits = 11 if form == "f16" else 8
    for b, s4 in enumerate(inp["scales"]):
        if not any(s4):
            continue
        f = factors(inp["aor"], inp["col"], s4).double()
        T = X[b] @ A.t()
        Ts = T * f
        ref[b] = Y[b] + Ts @ Bm.t()
        ts_term = _half_ulp(Ts.abs(), 8) @ Bm.abs().t()
        S = Y[b].abs() + ((X[b].abs() @ A.abs().t()) * f.abs()) @ Bm.abs().t()
        acc_term = acc_units * 2.0 ** -24 * S
        bar[b] = _half_ulp(ref[b].abs() + ts_term + acc_term, out_bits) + ts_term + acc_term
    return ref, bar


def emulate(inp, form, *, mutant=None, roundings=True):
    """An honest kernel on the CPU -> [B, rows, N] in the output type: T accumulated in fp32 over 32-wide contraction steps (each step's
    products summed exactly, as one MFMA does to well below an fp32 ulp), Ts = bf16(f T) with the fp32 factor applied first, the second
    product likewise over 32 rank columns, fp32(Y) + that, ONE rounding.  mutant: 'neighbour_scale' (the next stream's scales),
    'no_alpha_over_rank', 'scale_after_rounding' (bf16(f bf16(T))), 'pad_column_as_data' (pad rank columns hold data and a factor),
    'headpad_rows_nonzero', 'no_qscale', 'untransposed' (the term of the transposed form laid out row-major)."""
    X, Y = inp["X"], inp["Y"]
    A, Bm, aor = inp["down"].clone(), inp["up"].clone(), inp["aor"].clone()
    g = torch.Generator().manual_seed(5)
    if mutant == "pad_column_as_data":
        pc = inp["pad_cols"]
        A[pc] = bf(torch.randn(int(pc.sum()), A.shape[1], generator=g) / math.sqrt(A.shape[1]))
        Bm[:, pc] = bf(torch.randn(Bm.shape[0], int(pc.sum()), generator=g))
        aor[pc] = 1.0
    if mutant == "headpad_rows_nonzero":
        pr = inp["pad_rows"]
        Bm[pr] = bf(torch.randn(int(pr.sum()), Bm.shape[1], generator=g))
    if mutant == "no_qscale":
        Bm = inp["up_raw"].clone()
    if mutant == "no_alpha_over_rank":
        aor = (~inp["pad_cols"]).float()
    out = Y.clone() if roundings else Y.float()
    nb = len(inp["scales"])

    def steps(P, Q):                                                  # P [m, c] Q [n, c] -> fp32 [m, n], accumulated over 32-wide steps of c
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
        term = steps(Ts, Bm)
        if mutant == "untransposed":
            term = term.reshape(term.shape[1], term.shape[0]).t()
        out[b] = (Y[b].float() + term).to(Y.dtype if roundings else torch.float32)
    return out


def worst_and_share(got, ref, bar):
    """(largest |got - ref| / bar, share of elements above 1) over the elements with a bar (the adapted streams)."""
    m = bar > 0
    ratio = (got.double() - ref).abs()[m] / bar[m]
    return ratio.max().item(), (ratio > 1).double().mean().item()


def measured_acc_units(case):
    """The worst error of the honest emulation's fp32 arithmetic ALONE - the emulation without its two roundings, everything else as it
    is - against fp64, in units of 2^-24 S (see the module docstring)."""
    inp = op_inputs(case)
    X, Y, A, Bm = inp["X"].double(), inp["Y"].double(), inp["down"].double(), inp["up"].double()
    got = emulate(inp, case["form"], roundings=False).double()
    worst = 0.0
    for b, s4 in enumerate(inp["scales"]):
        if not any(s4):
            continue
        f = factors(inp["aor"], inp["col"], s4).double()
        ref = Y[b] + ((X[b] @ A.t()) * f) @ Bm.t()
        S = Y[b].abs() + ((X[b].abs() @ A.abs().t()) * f.abs()) @ Bm.abs().t()
        worst = max(worst, ((got[b] - ref).abs() / (2.0 ** -24 * S)).max().item())
    return worst


# ---------------------------------------------------------------------------------------------------------------- the oracle
def merged_sd(sd, checkpoints, scales):
    """The UNet state dict a stream with adapter scales `scales` is equivalent to: lora.merge_lora per adapter at that stream's scale."""
    from rich_text_to_image_amd.lora import merge_lora
    out = sd
    for ck, s in zip(checkpoints, scales):
        if s != 0:
            out, _ = merge_lora(out, ck, s)
    return out


def lora_oracle(cfg, sd, checkpoints, scales_per_forward):
    """An OracleUNet (oracle/unet.py, unchanged) whose k-th forward() call runs with the weights merged at scales_per_forward[k]."""
    from oracle.unet import OracleUNet

    class LoraOracleUNet(OracleUNet):
        def __init__(self):
            super().__init__(cfg, sd)
            memo = {}
            self.sds = []
            for s in scales_per_forward:
                key = tuple(float(v) for v in s)
                if key not in memo:
                    memo[key] = {k: v.detach().float() for k, v in merged_sd(sd, checkpoints, key).items()}
                self.sds.append(memo[key])
            self.calls = 0

        def forward(self, *a, **kw):
            self.sd = self.sds[self.calls]
            self.calls += 1
            return super().forward(*a, **kw)
    return LoraOracleUNet()


# ---------------------------------------------------------------------------------------------------------------- checkpoints
ATTN_LEAVES = ("to_q", "to_k", "to_v", "to_out.0")


def attention_projections(sd):
    """The module paths of the eight attention projections of every transformer block of a UNet state dict, in its order."""
    return [k[:-7] for k in sd if k.endswith(".weight") and ".transformer_blocks." in k and any(k.endswith(f".attn{a}.{l}.weight") for a in (1, 2) for l in ATTN_LEAVES)]


def synthetic_adapter(sd, rank=4, alpha=None, seed=0, layout="kohya", gain=1.0, extra=()):
    """A LoRA checkpoint on the attention projections of `sd`: down uniform(+-1 / sqrt(K)), up uniform(+-gain / sqrt(rank)), so that at
    alpha = rank the delta is of the weights' own size times `gain`.  layout: 'kohya' (with .alpha), 'peft', 'diffusers' (>= 0.20),
    'diffusers018' (attention-processor names).  extra: further module paths of `sd` to adapt (for the refusals).
    -> (checkpoint, {module path: (down, up, alpha)})."""
    g = torch.Generator().manual_seed(seed)
    ck, truth = {}, {}
    for path in list(attention_projections(sd)) + list(extra):
        W = sd[path + ".weight"]
        N, K = W.shape[0], W[0].numel()
        down = (torch.rand(rank, K, generator=g) * 2 - 1) / math.sqrt(K)
        up = (torch.rand(N, rank, generator=g) * 2 - 1) * gain / math.sqrt(rank)
        a = float(rank if alpha is None else alpha)
        truth[path] = (down, up, a)
        if W.dim() == 4:
            down, up = down.reshape(rank, *W.shape[1:]), up.reshape(N, rank, 1, 1)
        if layout == "kohya":
            m = "lora_unet_" + path.replace(".", "_")
            ck[m + ".lora_down.weight"], ck[m + ".lora_up.weight"], ck[m + ".alpha"] = down, up, torch.tensor(a)
        elif layout == "peft":
            assert alpha is None, "the peft layout stores no alpha"
            ck[f"unet.{path}.lora_A.weight"], ck[f"unet.{path}.lora_B.weight"] = down, up
        elif layout == "diffusers":
            assert alpha is None
            ck[f"unet.{path}.lora.down.weight"], ck[f"unet.{path}.lora.up.weight"] = down, up
        else:
            assert layout == "diffusers018" and alpha is None
            head, leaf = path.rsplit(".attn", 1)
            attn, proj = ("attn" + leaf).split(".", 1)
            proj = "to_out" if proj == "to_out.0" else proj
            ck[f"unet.{head}.{attn}.processor.{proj}_lora.down.weight"], ck[f"unet.{head}.{attn}.processor.{proj}_lora.up.weight"] = down, up
    return ck, truth
