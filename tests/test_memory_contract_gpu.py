"""The memory contract of every kernel route through the C ABI: where a kernel reads and writes, not what it computes.

Every case runs twice.  Run (a) is plain: contiguous operands, exact allocations.  Run (b) is the contract run (tests/memguard.py):
every output is a window of a wider buffer between two guard bands (leading dimension larger than its width wherever the entry point
takes one), pre-filled with NaN; every input sits in such a window whose padding columns and guards ARE NaN.  The contract run goes
first, and its guards are checked before the plain run starts.  Asserted, in this order:

  1. intact         not a byte outside an output window changed (both guards, the padding columns of every row)
  2. fully written  the window holds no NaN: every element was written, and no NaN of an input's surroundings was read into it
  3. bit-equal      (b) equals (a) bit for bit - the route is a function of the shape, never of a leading dimension (asked through
                    rt_op_gemm_route for both argument sets)
  4. reference      (a) against an fp64 evaluation of the operator on the same rounded inputs, at the bars tests/test_kernels_gpu.py
                    uses for that kernel and output type (set against fp32 references of larger problems)

Memory INSIDE an operand's declared extent that the contract calls "anything finite" (cross-attention K / V rows behind a prompt's keys)
holds alternating-sign junk of magnitude 1e3, not NaN; NaN goes only where a kernel must not look.

Shapes are the smallest that reach the route (tests/memcases.py, checked on the CPU by tests/test_gemm_route.py) with a ragged last row
tile and, where the kernel allows, a ragged last column chunk and K tail.  The precise VAE's hi / lo routes (TRIPLE and the three-pass
kernels) and the VAE's other kernels get the same contract in tests/test_vae_ops_gpu.py, through rt_op_gemm_hilo and its siblings.
"""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hiputil import DEV, attention, bf, chk, gemm, report, small_linear  # noqa: E402
from memcases import (G16_K, G16_M, G16_VARIANT_CASES, GEMM_CASES, KIND_NAMES, UPCONV_CASES, case_id, conv_out_hw,  # noqa: E402
                      route_args)
from memguard import damage, guarded, intact, poisoned, unwritten  # noqa: E402

BF16_OUT = dict(atol=2e-2, rtol=1.2e-2)
F32_OUT = dict(atol=2e-3, rtol=2e-3)
F16_OUT = dict(atol=4e-3, rtol=1.5e-3)
ATTN = dict(atol=1.5e-2, rtol=1.5e-2)
EPI_TOL = {0: BF16_OUT, 1: F32_OUT, 2: BF16_OUT, 3: BF16_OUT, 4: F16_OUT}
EPI_DTYPE = {0: torch.bfloat16, 1: torch.float32, 2: torch.bfloat16, 3: torch.bfloat16, 4: torch.float16}
PAD = 8                 # extra columns of every padded leading dimension: keeps the launchers' multiples (8 for 16-bit operands, 4 for fp32) and 16-byte rows
LN2 = math.log(2.0)


def _lib():
    from rich_text_to_image_amd.engine import load_library
    return load_library()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def junk(*shape):
    """Finite junk for memory an operand declares but a kernel must mask: +-1e3, alternating."""
    n = 1
    for s in shape:
        n *= s
    i = torch.arange(n, dtype=torch.float32)
    return ((1000.0 + (i % 7)) * (1.0 - 2.0 * (i % 2))).reshape(shape)


def dd(t):
    return t.to(DEV).double()


def pz(t, ld=None):
    """poisoned(), None passes through; 2-D operands get PAD extra columns unless ld says otherwise (ld = 0: no padding columns)."""
    if t is None:
        return None
    if t.dim() == 2:
        return poisoned(t, t.shape[1] + PAD if ld is None else (ld or None))
    return poisoned(t)


def out_window(rows, cols, dtype, pad=PAD):
    return guarded((rows, cols), dtype, ld=cols + pad, device=DEV)


def check_windows(name, windows):
    """Assertions 1 and 2 of the module docstring over [(label, big, win)], each over every output before the next.  Every test makes
    its contract run FIRST and calls this before the plain run: a kernel that strays is then stopped where the stray lands in a guard
    band, before it runs on exact allocations."""
    torch.cuda.synchronize()
    for label, big, win in windows:
        assert intact(big, win), f"{name}: stray write around {label}: {damage(big, win)}"
    for label, _, win in windows:
        n = unwritten(win)
        assert n == 0, f"{name}: {n} of {win.numel()} elements of {label} are not finite (never written, or NaN read from an input's surroundings)"


def check_equal(name, pairs):
    """Assertion 3 over [(label, win, plain)]."""
    for label, win, plain in pairs:
        p = plain.reshape(win.shape)
        assert torch.equal(win, p), f"{name}: {label} differs between the plain and the contract run: max {(win.float() - p.float()).abs().max().item():.4e}"


def nans(rows, cols, dtype=torch.float32):
    return torch.full((rows, cols), float("nan"), device=DEV, dtype=dtype)


class switches:
    def __init__(self, cfg=-1, debug=0):
        self.cfg, self.debug = cfg, debug

    def __enter__(self):
        lib = _lib()
        assert lib.rt_op_gemm_force_config(self.cfg) == 0
        lib.rt_op_gemm_debug(self.debug)

    def __exit__(self, *exc):
        lib = _lib()
        lib.rt_op_gemm_force_config(-1)
        lib.rt_op_gemm_debug(0)


def geglu_rows(half):
    """The engine's GEGLU packing (test_gemm_geglu_epilogue): per 64-row block [32 value rows | 32 gate rows]."""
    rows = []
    for blk in range(half // 32):
        rows += list(range(blk * 32, blk * 32 + 32)) + list(range(half + blk * 32, half + blk * 32 + 32))
    return rows


def im2col64(x, mode, Hout, Wout):
    """fp64 [B, H, W, C] -> [B * Hout * Wout, 9 C], K index = tap * C + c (ky major): the 3x3 convolution as a plain matrix product."""
    if mode == 3:
        x = x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)
    st = 2 if mode == 2 else 1
    B, H, W, Cc = x.shape
    xp = torch.zeros(B, H + 2, W + 2, Cc, dtype=x.dtype, device=x.device)
    xp[:, 1:H + 1, 1:W + 1] = x
    taps = [xp[:, ky:ky + st * (Hout - 1) + 1:st, kx:kx + st * (Wout - 1) + 1:st] for ky in range(3) for kx in range(3)]
    return torch.cat(taps, dim=-1).reshape(B * Hout * Wout, 9 * Cc)


def epilogue_operands(epi, M, N, nb, bias, seed):
    """(bias, res, temb) of an epilogue on the device, and what they add to the fp64 reference [M, N]."""
    b = rnd(N, seed=seed).to(DEV) if bias else None
    res = temb = None
    add = torch.zeros(M, N, dtype=torch.float64, device=DEV)
    if b is not None:
        add += b.double()
    if epi == 1:
        res = rnd(M, N, seed=seed + 1).to(DEV)
    if epi == 4:
        res = (rnd(M, N, seed=seed + 1) * 3).to(DEV).to(torch.float16)
    if res is not None:
        add += res.double()
    if epi == 2:
        temb = rnd(nb, N, seed=seed + 2).to(DEV)
        add += temb.double().repeat_interleave(M // nb, dim=0)
    return b, res, temb, add


# ----------------------------------------------------------------------------------------------- rt_op_gemm: dense and 3x3 convolutions, every route
def _route(args):
    k, v, s = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    assert _lib().rt_op_gemm_route(*args, C.byref(k), C.byref(v), C.byref(s)) == 0
    return k.value, v.value, s.value


@pytest.mark.parametrize("case", GEMM_CASES, ids=case_id)
def test_gemm_route_memory_contract(case):
    c, epi, name = case, case["epi"], case_id(case)
    if c["mode"] == 0:
        M, N, K = c["M"], c["N"], c["K"]
        A = bf(rnd(M, K, seed=1))
        nb, conv = (M // c["rpb"] if c["rpb"] else 1), None
        a64 = A.double()
    else:
        Ho, Wo = conv_out_hw(c)
        M, N, K = c["B"] * Ho * Wo, c["Cout"], 9 * c["Cin"]
        A = bf(rnd(c["B"], c["H"], c["W"], c["Cin"], seed=1))          # NHWC: no leading dimension - NaN guards on either side
        nb, conv = c["B"], (Ho, Wo)
        a64 = im2col64(A.double(), c["mode"], Ho, Wo)
    Wfull = rnd(N, K, seed=2, scale=K ** -0.5)
    bias, res, temb, add = epilogue_operands(epi, M, N, nb, c["bias"], seed=3)
    if epi == 3:
        rows = geglu_rows(N // 2)
        W = bf(Wfull[rows])
        bias_k = bias[rows].contiguous() if bias is not None else None
        h = a64 @ bf(Wfull).double().t() + add
        a_, g_ = h.chunk(2, dim=-1)
        ref = a_ * F.gelu(g_)
    else:
        W, bias_k = bf(Wfull), bias
        ref = a64 @ W.double().t() + add
    oc = ref.shape[1]
    kw = dict(epi=epi, mode=c["mode"], conv=conv, rows_per_batch=c.get("rpb", 0))
    with switches(c["cfg"], c["debug"]):
        ra, rb = _route(route_args(c)), _route(route_args(c, pad=PAD))
        assert ra == rb and ra[0] == c["kind"], f"{name}: routes {KIND_NAMES[ra[0]]} / {KIND_NAMES[rb[0]]}"
        big, win = out_window(M, oc, EPI_DTYPE[epi])
        gemm(pz(A), pz(W), pz(bias_k), res=pz(res, res.shape[1] + (PAD if epi == 4 else 4)) if res is not None else None,
             temb=pz(temb, N + 4), out=win, **kw)
        check_windows(name, [("out", big, win)])
        plain = gemm(A, W, bias_k, res=res, temb=temb, **kw)
    check_equal(name, [("out", win, plain)])
    report(name, plain, ref, **EPI_TOL[epi])


# ----------------------------------------------------------------------------------------------- rt_op_gemm16_variant: the tiles of gemm16.hip by name
def _gemm16(A, W, bias, epi, variant, res, wstat, vt, out):
    lib = _lib()
    M, K = A.shape
    N = W.shape[0]
    chk(lib.rt_op_gemm16_variant(_ptr(A), _ptr(W), _ptr(bias), _ptr(out), _ptr(res), epi, M, N, K, A.stride(0), W.stride(0), out.stride(0),
                                 res.stride(0) if res is not None else 0, vt, variant, wstat, None))
    torch.cuda.synchronize()
    return out


G16_RUNS = [(v, N, vt, e, 0) for v, N, vt, epis in G16_VARIANT_CASES for e in epis] + [(2, 2048, 0, 3, 1), (8, 2048, 0, 3, 1)]   # the W-stationary tile order (8 column tiles)


@pytest.mark.parametrize("variant,N,vt,epi,wstat", G16_RUNS, ids=lambda v: str(v))
def test_gemm16_variant_memory_contract(variant, N, vt, epi, wstat):
    """M = 300 rows (every tile height ragged), K = 256, all four leading dimensions padded.  The V^T variants take the weights on the rows:
    320 weight rows x 296 token columns (a bf16 row of tokens is whole 16-byte chunks), ragged against the 224- / 128- / 64-column tiles."""
    M, K = (320, G16_K) if vt else (G16_M, G16_K)
    name = f"gemm16 variant {variant} {M}x{N}x{K} epi{epi} wstat{wstat} vt{vt}"
    A = bf(rnd(M, K, seed=1, scale=K ** -0.5 if vt else 1.0))
    Wfull = rnd(N, K, seed=2, scale=1.0 if vt else K ** -0.5)
    bias, res, _, add = epilogue_operands(epi, M, N, 1, not vt, seed=3)
    if epi == 3:
        rows = geglu_rows(N // 2)
        W, bias_k = bf(Wfull[rows]), bias[rows].contiguous()
        a_, g_ = (A.double() @ bf(Wfull).double().t() + add).chunk(2, dim=-1)
        ref = a_ * F.gelu(g_)
    else:
        W, bias_k = bf(Wfull), bias
        ref = A.double() @ W.double().t() + add
    oc = ref.shape[1]
    big, win = out_window(M, oc, EPI_DTYPE[epi])
    _gemm16(pz(A), pz(W), pz(bias_k), epi, variant, pz(res, N + (PAD if epi == 4 else 4)) if res is not None else None, wstat, vt, win)
    check_windows(name, [("out", big, win)])
    plain = _gemm16(A, W, bias_k, epi, variant, res, wstat, vt, nans(M, oc, EPI_DTYPE[epi]))
    check_equal(name, [("out", win, plain)])
    report(name, plain, ref, **EPI_TOL[epi])


# ----------------------------------------------------------------------------------------------- rt_op_gemm_qk_vt: grouped and as two launches
@pytest.mark.parametrize("debug", [0, 1 << 13], ids=["grouped", "two-launches"])
def test_qk_vt_pair_memory_contract(debug):
    """attn1's two projections at the smallest shape with Mqk < M that rt_op_gemm_pair_pick admits (5 of 6 streams of 768 tokens, 640 ->
    1280 channels): ldx, ldqk and ldvt padded, both outputs guarded - the Q|K rows behind Mqk belong to nobody and stay untouched."""
    lib = _lib()
    sqk, s, rps, Cc, HD = 5, 6, 768, 640, 1280
    assert lib.rt_op_gemm_pair_pick(sqk, s, rps, 2 * HD, HD, Cc) >= 0
    M, Mqk = s * rps, sqk * rps
    X = bf(rnd(M, Cc, seed=1))
    Wqk, Wv = bf(rnd(2 * HD, Cc, seed=2, scale=Cc ** -0.5)), bf(rnd(HD, Cc, seed=3, scale=Cc ** -0.5))
    bqk = rnd(2 * HD, seed=4).to(DEV)

    def run(X_, Wqk_, bqk_, Wv_, qk, vt):
        grouped = C.c_int(-1)
        lib.rt_op_gemm_debug(debug)
        try:
            chk(lib.rt_op_gemm_qk_vt(_ptr(X_), X_.stride(0), Cc, rps, _ptr(Wqk_), _ptr(bqk_), Mqk, 2 * HD, _ptr(qk), qk.stride(0), _ptr(Wv_), HD, M,
                                     _ptr(vt), vt.stride(0), C.byref(grouped), None))
        finally:
            lib.rt_op_gemm_debug(0)
        torch.cuda.synchronize()
        assert grouped.value == (0 if debug else 1)
    bq, qk_b = out_window(Mqk, 2 * HD, torch.bfloat16)
    bv, vt_b = out_window(HD, M, torch.bfloat16)
    # Wqk / Wv have no leading dimension of their own (ldw = K): guards only
    run(pz(X), pz(Wqk, 0), pz(bqk), pz(Wv, 0), qk_b, vt_b)
    check_windows(f"qk_vt debug {debug:x}", [("qk", bq, qk_b), ("vt", bv, vt_b)])
    qk_a, vt_a = nans(Mqk, 2 * HD, torch.bfloat16), nans(HD, M, torch.bfloat16)
    run(X, Wqk, bqk, Wv, qk_a, vt_a)
    check_equal(f"qk_vt debug {debug:x}", [("qk", qk_b, qk_a), ("vt", vt_b, vt_a)])
    report("Q|K", qk_a, X[:Mqk].double() @ Wqk.double().t() + bqk.double(), **BF16_OUT)
    report("V^T", vt_a, Wv.double() @ X.double().t(), **BF16_OUT)


# ----------------------------------------------------------------------------------------------- rt_op_upconv: the four-phase launch and the patch kernel
def test_upconv_memory_contract():
    """The phase route (G16_UP2) at the smallest shape with *phase_route == 1, and the same call without the phase pack (patch kernel):
    input between NaN guards, output guarded.  The two outputs are compared as tests/test_upconv_subpixel_gpu.py does - each against
    F.conv2d(F.interpolate(x)) of the UNROUNDED weights in fp64, rel-L2(phase) <= 1.1 x rel-L2(patch), whole map and borders - because
    the phase weights are sums rounded once, not the nine rounded taps."""
    lib = _lib()
    B, H, W_, Cin, Cout = UPCONV_CASES[0][:5]
    x = rnd(B, H, W_, Cin, seed=31).to(torch.bfloat16)
    w = rnd(Cout, Cin, 3, 3, seed=32, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=33).to(DEV)
    A, w9 = x.to(DEV).contiguous(), bf(w.permute(0, 2, 3, 1).reshape(Cout, -1))
    wd = w.to(DEV).contiguous()
    wph = torch.full((4, Cout, 4 * Cin), float("nan"), device=DEV, dtype=torch.bfloat16)
    chk(lib.rt_op_pack_upconv(_ptr(wd), 0, Cout, Cin, _ptr(wph), None))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(wph.float()).all())
    M = B * 4 * H * W_
    ref = im2col64(A.double(), 3, 2 * H, 2 * W_) @ dd(w.permute(0, 2, 3, 1).reshape(Cout, -1)).t() + bias.double()
    outs = {}
    for _, _, _, _, _, with_pack, expect in UPCONV_CASES:
        def run(A_, w9_, wph_, bias_, out):
            route = C.c_int(-1)
            chk(lib.rt_op_upconv(_ptr(A_), _ptr(w9_), _ptr(wph_), _ptr(bias_), _ptr(out), B, H, W_, Cin, Cout, C.byref(route), None))
            torch.cuda.synchronize()
            assert route.value == expect
        big, win = guarded((M, Cout), torch.float16, device=DEV)          # rt_op_upconv takes no ldo: guards only
        run(pz(A), pz(w9, 0), pz(wph) if with_pack else None, pz(bias), win)
        check_windows(f"upconv phase_route {expect}", [("out", big, win)])
        plain = nans(M, Cout, torch.float16)
        run(A, w9, wph if with_pack else None, bias, plain)
        check_equal(f"upconv phase_route {expect}", [("out", win, plain)])
        outs[expect] = plain

    def rel_l2(a, b):
        return ((a.double() - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()
    e_new, e_old = rel_l2(outs[1], ref), rel_l2(outs[0], ref)
    edge = torch.zeros(2 * H, 2 * W_, dtype=torch.bool, device=DEV)
    edge[:2] = edge[-2:] = True
    edge[:, :2] = edge[:, -2:] = True
    sel = edge.reshape(-1).repeat(B)
    b_new, b_old = rel_l2(outs[1][sel], ref[sel]), rel_l2(outs[0][sel], ref[sel])
    print(f"upconv rel-L2 vs fp64 of the unrounded weights: phase {e_new:.4e} patch {e_old:.4e}; borders {b_new:.4e} / {b_old:.4e}")
    assert e_new <= 1.1 * e_old and b_new <= 1.1 * b_old
    # the patch route multiplies the nine bf16-rounded taps: against fp64 of exactly those
    report("upconv patch route", outs[0], im2col64(A.double(), 3, 2 * H, 2 * W_) @ w9.double().t() + bias.double(), **F16_OUT)


# ----------------------------------------------------------------------------------------------- norms
def groupnorm64(x, G, gamma, beta, eps, silu):
    B, HW, Cc = x.shape
    v = x.double().reshape(B, HW, G, Cc // G)
    mean = v.mean(dim=(1, 3), keepdim=True)
    var = (v - mean).pow(2).mean(dim=(1, 3), keepdim=True)
    y = ((v - mean) / (var + eps).sqrt()).reshape(B, HW, Cc) * gamma.double() + beta.double()
    return F.silu(y) if silu else y


# (in_type, HW, C1, C2, G, raw, debug, form): one-launch and two-launch forms for each input type, the virtual concat, raw_out, HW that is
# no multiple of the chunk rows (96, 1008), B = 2; debug bit 23 forces the two-launch form with 8-wide loads on a one-launch shape
GN_CASES = [(2, 96, 1280, 1280, 32, True, 0, 1), (2, 1008, 640, 0, 32, False, 0, 1), (0, 96, 64, 0, 8, True, 0, 1), (1, 1008, 64, 0, 8, False, 0, 1),
            (2, 1008, 1280, 0, 32, True, 0, 1),
            (2, 96, 320, 0, 32, True, 0, 2), (2, 1008, 36, 36, 4, False, 0, 2), (0, 96, 40, 32, 4, True, 0, 2), (1, 1008, 40, 0, 4, False, 0, 2),
            (2, 96, 1280, 1280, 32, True, 1 << 23, 2), (0, 1008, 64, 64, 8, False, 1 << 23, 2)]


@pytest.mark.parametrize("in_type,HW,C1,C2,G,raw,debug,form", GN_CASES)
def test_groupnorm_memory_contract(in_type, HW, C1, C2, G, raw, debug, form):
    lib = _lib()
    B, Cc = 2, C1 + C2
    dt = {0: torch.float32, 1: torch.bfloat16, 2: torch.float16}[in_type]
    x1 = (rnd(B, HW, C1, seed=60) * 2 + 0.5).to(dt).to(DEV)
    x2 = (rnd(B, HW, C2, seed=61) - 0.3).to(dt).to(DEV) if C2 else None
    gamma, beta = (1 + 0.1 * rnd(Cc, seed=62)).to(DEV), (0.1 * rnd(Cc, seed=63)).to(DEV)
    name = f"groupnorm type{in_type} HW{HW} C{C1}+{C2} G{G} form{form}"

    def run(x1_, x2_, gamma_, beta_, out, raw_out):
        lib.rt_op_gemm_debug(debug)
        try:
            assert lib.rt_op_groupnorm_form(in_type, C1, C2, G, B, HW) == form
            chk(lib.rt_op_groupnorm(_ptr(x1_), _ptr(x2_), in_type, C1, C2, G, B, HW, _ptr(gamma_), _ptr(beta_), C.c_float(1e-5), 1, _ptr(out),
                                    _ptr(raw_out), None))
        finally:
            lib.rt_op_gemm_debug(0)
        torch.cuda.synchronize()
    bo, out_b = guarded((B * HW, Cc), torch.bfloat16, device=DEV)
    br, raw_b = guarded((B * HW, Cc), torch.bfloat16, device=DEV) if raw else (None, None)
    run(pz(x1), pz(x2), pz(gamma), pz(beta), out_b, raw_b)
    check_windows(name, [("out", bo, out_b)] + ([("raw", br, raw_b)] if raw else []))
    out_a, raw_a = nans(B * HW, Cc, torch.bfloat16), nans(B * HW, Cc, torch.bfloat16) if raw else None
    run(x1, x2, gamma, beta, out_a, raw_a)
    check_equal(name, [("out", out_b, out_a)] + ([("raw", raw_b, raw_a)] if raw else []))
    xc = torch.cat([x1, x2], -1) if C2 else x1
    report(name, out_a, groupnorm64(xc, G, gamma, beta, 1e-5, True).reshape(B * HW, Cc), **BF16_OUT)
    if raw:
        report(name + " raw copy", raw_a, xc.double().reshape(B * HW, Cc), atol=1e-2, rtol=8e-3)


@pytest.mark.parametrize("f16", [False, True], ids=["f32", "f16"])
@pytest.mark.parametrize("rows,Cc", [(77, 320), (515, 320), (77, 640), (515, 640), (77, 1536), (515, 1536)])
def test_layernorm_memory_contract(rows, Cc, f16):
    lib = _lib()
    x = (rnd(rows, Cc, seed=70) * 3 + 1).to(DEV)
    x = x.to(torch.float16) if f16 else x
    gamma, beta = (1 + 0.1 * rnd(Cc, seed=71)).to(DEV), (0.1 * rnd(Cc, seed=72)).to(DEV)
    fn = lib.rt_op_layernorm_f16 if f16 else lib.rt_op_layernorm

    def run(x_, g_, b_, out):
        chk(fn(_ptr(x_), _ptr(g_), _ptr(b_), _ptr(out), rows, Cc, C.c_float(1e-5), None))
        torch.cuda.synchronize()
    big, win = guarded((rows, Cc), torch.bfloat16, device=DEV)
    run(pz(x, 0), pz(gamma), pz(beta), win)
    check_windows(f"layernorm {rows}x{Cc}", [("out", big, win)])
    plain = nans(rows, Cc, torch.bfloat16)
    run(x, gamma, beta, plain)
    check_equal(f"layernorm {rows}x{Cc}", [("out", win, plain)])
    v = x.double()
    mean, var = v.mean(-1, keepdim=True), v.var(-1, unbiased=False, keepdim=True)
    report(f"layernorm {rows}x{Cc} f16={f16}", plain, (v - mean) / (var + 1e-5).sqrt() * gamma.double() + beta.double(), **BF16_OUT)


# ----------------------------------------------------------------------------------------------- LayerNorm fold: producer, stand-alone producer, consumers
def _partials64(xb, bn):
    rows = xb.shape[0]
    v = xb.double().reshape(rows, -1, bn)
    t = torch.stack([v.sum(-1), (v * v).sum(-1)], dim=-1)
    return t.reshape(rows, -1, 4).permute(1, 0, 2).contiguous()


def _trunk(tokens, Cw, seed):
    x = rnd(tokens, Cw, seed=seed) * (0.5 + rnd(tokens, 1, seed=seed + 1).abs() * 2) + rnd(tokens, 1, seed=seed + 2)
    return (x + rnd(1, Cw, seed=seed + 3) * 0.5).to(DEV).to(torch.float16).contiguous()


@pytest.mark.parametrize("rows,Cw,bn", [(300, 640, 160), (300, 640, 320), (77, 1280, 160), (515, 1280, 320)])
def test_ln_partials_memory_contract(rows, Cw, bn):
    lib = _lib()
    x = _trunk(rows, Cw, seed=11)
    npair = Cw // bn // 2

    def run(x_, xb, part):
        chk(lib.rt_op_ln_partials(_ptr(x_), _ptr(xb), _ptr(part), rows, Cw, bn, None))
        torch.cuda.synchronize()
    bx, xb_b = guarded((rows, Cw), torch.bfloat16, device=DEV)
    bp, part_b = guarded((npair * rows, 4), torch.float32, device=DEV)
    run(pz(x, 0), xb_b, part_b)
    check_windows(f"ln_partials {rows}x{Cw}/{bn}", [("xb", bx, xb_b), ("partials", bp, part_b)])
    xb_a, part_a = nans(rows, Cw, torch.bfloat16), nans(npair * rows, 4)
    run(x, xb_a, part_a)
    check_equal(f"ln_partials {rows}x{Cw}/{bn}", [("xb", xb_b, xb_a), ("partials", part_b, part_a)])
    assert torch.equal(xb_a, x.to(torch.bfloat16))
    ref = _partials64(xb_a, bn).reshape(npair * rows, 4)
    assert torch.allclose(part_a.double(), ref, rtol=2e-6, atol=2e-3), (part_a.double() - ref).abs().max().item()      # test_lnfold_gpu.py's bar


def test_gemm_emit_partials_memory_contract():
    """The trunk-producing GEMM that also leaves xb and the LayerNorm partials, at test_lnfold_gpu.py's smallest shape: out, xb and partials
    guarded, operands between NaN guards (the entry point takes no leading dimensions)."""
    lib = _lib()
    M, N, K, rps = 2048, 1280, 1280, 1024
    A, W = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2, scale=K ** -0.5))
    bias = rnd(N, seed=3).to(DEV)
    res = (rnd(M, N, seed=4) * 3 + rnd(M, 1, seed=5) * 2).to(DEV).to(torch.float16)
    bns = []

    def run(A_, W_, bias_, res_, out, xb, part):
        bn = C.c_int(0)
        chk(lib.rt_op_gemm_emit_partials(_ptr(A_), _ptr(W_), _ptr(bias_), _ptr(out), _ptr(res_), M, N, K, rps, _ptr(xb), _ptr(part), C.byref(bn), None))
        torch.cuda.synchronize()
        assert bn.value in (160, 320)
        bns.append(bn.value)
    bo, out_b = guarded((M, N), torch.float16, device=DEV)
    bx, xb_b = guarded((M, N), torch.bfloat16, device=DEV)
    bp, part_all = guarded((4 * M, 4), torch.float32, device=DEV)           # room for 160-column tiles; the launch owns N / bn / 2 pair planes of M rows
    run(pz(A, 0), pz(W, 0), pz(bias), pz(res, 0), out_b, xb_b, part_all)
    used = N // bns[0] // 2 * M
    part_b = part_all[:used]
    assert intact(bp, part_all) and bool(torch.isnan(part_all[used:]).all()), "partials: a write outside the pair planes the launch owns"
    check_windows("gemm_emit_partials", [("out", bo, out_b), ("xb", bx, xb_b)])
    assert unwritten(part_b) == 0
    out_a, xb_a, part_a = nans(M, N, torch.float16), nans(M, N, torch.bfloat16), nans(4 * M, 4)
    run(A, W, bias, res, out_a, xb_a, part_a)
    assert bns[0] == bns[1]
    check_equal("gemm_emit_partials", [("out", out_b, out_a), ("xb", xb_b, xb_a), ("partials", part_b, part_a[:used])])
    report("emit trunk", out_a, A.double() @ W.double().t() + bias.double() + res.double(), **F16_OUT)
    assert torch.allclose(xb_a.float(), out_a.float(), rtol=2.0 ** -7, atol=1e-4)
    ref = _partials64(xb_a, bns[0]).reshape(used, 4)
    assert torch.allclose(part_a[:used].double(), ref, rtol=2e-6, atol=2e-3), (part_a[:used].double() - ref).abs().max().item()


@pytest.mark.parametrize("form", ["epi0", "vt", "geglu"])
def test_ln_gemm_memory_contract(form):
    """The folded consumers at test_lnfold_gpu.py's smallest shape (2 streams x 1024 tokens x 1280 channels), fed from the fp16 trunk:
    output guarded, operands between NaN guards.  Reference: fp64 layer_norm(x) W^T + b at that module's per-row tolerance (report_rows:
    the fold multiplies bf16(x), not bf16(LN(x)))."""
    from test_lnfold_gpu import report_rows
    lib = _lib()
    tokens, Cw, rps = 2048, 1280, 1024
    x = _trunk(tokens, Cw, seed=11)
    gamma, beta = (1.0 + 0.3 * rnd(Cw, seed=12)).to(DEV), (0.2 * rnd(Cw, seed=13)).to(DEV)
    v = x.double()
    ln = (v - v.mean(-1, keepdim=True)) / (v.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt() * gamma.double() + beta.double()
    vt, epi, geglu = form == "vt", 3 if form == "geglu" else 0, None
    if form == "geglu":
        N = 8 * Cw
        Wfull, bfull = rnd(N, Cw, seed=41, scale=Cw ** -0.5), rnd(N, seed=42)
        rows = geglu_rows(N // 2)
        W, b = bf(Wfull[rows]), bfull[rows].to(DEV).contiguous()
        a_, g_ = (ln @ bf(Wfull).double().t() + dd(bfull)).chunk(2, dim=-1)
        ref, geglu, shape = a_ * F.gelu(g_), (a_, g_), (tokens, N // 2)
    elif vt:
        N = Cw
        W, b = bf(rnd(N, Cw, seed=31, scale=Cw ** -0.5)), None
        ref, shape = W.double() @ ln.t(), (N, tokens)
    else:
        N = Cw
        W, b = bf(rnd(N, Cw, seed=21, scale=Cw ** -0.5)), rnd(N, seed=121).to(DEV)
        ref, shape = ln @ W.double().t() + b.double(), (tokens, N)

    def run(x_, g_, be_, W_, b_, out):
        chk(lib.rt_op_ln_gemm(_ptr(x_), _ptr(g_), _ptr(be_), _ptr(W_), _ptr(b_), _ptr(out), tokens, N, Cw, epi, int(vt), rps, None, None, 160, None))
        torch.cuda.synchronize()
    big, win = guarded(shape, torch.bfloat16, device=DEV)
    run(pz(x, 0), pz(gamma), pz(beta), pz(W, 0), pz(b), win)
    check_windows(f"ln_gemm {form}", [("out", big, win)])
    plain = nans(*shape, torch.bfloat16)
    run(x, gamma, beta, W, b, plain)
    check_equal(f"ln_gemm {form}", [("out", win, plain)])
    report_rows(f"ln_gemm {form}", plain, ref, x, vt=vt, geglu=geglu, **BF16_OUT)


# ----------------------------------------------------------------------------------------------- attention
def attn64(Q, K, V, H, DP, nkeys=None, wabs=None, wsgn=None):
    """fp64 softmax(Q K^T) V of one batch entry.  Q [N, H * DP] pre-scaled by d^-1/2 log2 e (the kernels' exp2 domain), K / V [NK, H * DP];
    nkeys: keys behind it are masked; wabs / wsgn [NK]: the font-size softmax of attention_processor.py:386-401 (exponentials times |size|,
    probabilities times its sign)."""
    N, NK = Q.shape[0], K.shape[0] if nkeys is None else nkeys
    q, k, v = (t.double().reshape(t.shape[0], H, DP).permute(1, 0, 2) for t in (Q, K[:NK], V[:NK]))
    s = q @ k.transpose(1, 2) * LN2
    e = (s - s.max(-1, keepdim=True)[0]).exp()
    if wabs is not None:
        e = e * wabs[:NK].double()
    p = e / e.sum(-1, keepdim=True)
    if wsgn is not None:
        p = p * wsgn[:NK].double()
    return (p @ v).permute(1, 0, 2).reshape(N, H * DP)


@pytest.mark.parametrize("DP", [32, 64, 96, 160])
@pytest.mark.parametrize("N", [128, 72, 144])
def test_self_attention_memory_contract(DP, N):
    """B = 2, H = 2, the engine's layout: Q and K in ONE buffer (ldq = ldk = 2 H DP, K at column H DP), V^T with ldvt > B N and NaN
    behind column B N, ldo > H DP.  N = 128: whole 64-key tiles; 72 and 144: the ragged last tile, whose keys behind N are the next
    entry's keys for entry 0 and NaN for the last entry."""
    B, H = 2, 2
    HD = H * DP
    qs = DP ** -0.5 * math.log2(math.e)
    QK = bf(torch.cat([rnd(B * N, HD, seed=30) * qs, rnd(B * N, HD, seed=31)], dim=1))
    V = bf(rnd(B * N, HD, seed=32))
    VT = V.t().contiguous()
    QKp, VTp = pz(QK, 0), pz(VT)
    big, win = out_window(B * N, HD, torch.bfloat16)
    attention(QKp[:, :HD], QKp[:, HD:], VTp, B, H, N, N, DP, O=win)
    check_windows(f"self_attn DP{DP} N{N}", [("O", big, win)])
    plain = attention(QK[:, :HD], QK[:, HD:], VT, B, H, N, N, DP)
    check_equal(f"self_attn DP{DP} N{N}", [("O", win, plain)])
    ref = torch.cat([attn64(QK[b * N:(b + 1) * N, :HD], QK[b * N:(b + 1) * N, HD:], V[b * N:(b + 1) * N], H, DP) for b in range(B)])
    report(f"self_attn DP{DP} N{N}", plain, ref, **ATTN)


@pytest.mark.parametrize("mode", [0, 2])
def test_shared_probability_attention_memory_contract(mode):
    """One shared-probability launch (three streams attend with stream 3's Q / K): rt_op_gemm_debug bits 24 - 26 = the shape rule / units
    of up to four members in one launch."""
    lib = _lib()
    B, H, N, DP = 6, 2, 256, 64
    src = [0, 1, 2, 3, 3, 3]
    HD = H * DP
    qs = DP ** -0.5 * math.log2(math.e)
    QK = bf(torch.cat([rnd(B * N, HD, seed=43) * qs, rnd(B * N, HD, seed=44)], dim=1))
    V = bf(rnd(B * N, HD, seed=45))
    VT = V.t().contiguous()
    kw = dict(q_src=src, k_src=src, v_src=list(range(B)))
    lib.rt_op_gemm_debug(mode << 24)
    try:
        QKp, VTp = pz(QK, 0), pz(VT)
        big, win = out_window(B * N, HD, torch.bfloat16)
        attention(QKp[:, :HD], QKp[:, HD:], VTp, B, H, N, N, DP, O=win, **kw)
        check_windows(f"shared-probability attention mode {mode}", [("O", big, win)])
        plain = attention(QK[:, :HD], QK[:, HD:], VT, B, H, N, N, DP, **kw)
    finally:
        lib.rt_op_gemm_debug(0)
    check_equal(f"shared-probability attention mode {mode}", [("O", win, plain)])
    ref = torch.cat([attn64(QK[src[b] * N:(src[b] + 1) * N, :HD], QK[src[b] * N:(src[b] + 1) * N, HD:], V[b * N:(b + 1) * N], H, DP) for b in range(B)])
    report(f"shared-probability attention mode {mode}", plain, ref, **ATTN)


def _cross_inputs(B, H, N, DP, P, NK, counts, seed):
    """Q, the prompt caches K [P * NK, H DP] / V with +-1e3 junk behind every prompt's keys, and a plain + a font-size multiplier set with
    a negative, a zero and a large size."""
    HD = H * DP
    qs = DP ** -0.5 * math.log2(math.e)
    Q = bf(rnd(B * N, HD, seed=seed) * qs)
    Kp, Vp = junk(P, NK, HD), junk(P, NK, HD)
    kc, vc = rnd(P, NK, HD, seed=seed + 1), rnd(P, NK, HD, seed=seed + 2)
    for p in range(P):
        Kp[p, :counts[p]] = kc[p, :counts[p]]
        Vp[p, :counts[p]] = vc[p, :counts[p]]
    return Q, bf(Kp.reshape(P * NK, HD)), bf(Vp.reshape(P * NK, HD))


@pytest.mark.parametrize("debug", [0, 1 << 19], ids=["cross77", "generic"])
@pytest.mark.parametrize("N", [64, 320])
def test_cross_attention_memory_contract(N, debug):
    """77-key cross-attention on cross77_kernel and (debug bit 19) the generic kernel: K / V rows 77..95 of every prompt hold finite
    junk (+-1e3) that must be masked, not multiplied by ~0; font sizes negative, zero and large; streams mix plain softmax without
    tables (wset -1), the plain table (0) and the font-size table (1); every leading dimension padded."""
    lib = _lib()
    B, H, DP, P = 3, 2, 64, 2
    HD = H * DP
    Q, K, V = _cross_inputs(B, H, N, DP, P, 96, [77] * P, seed=50)
    VT = V.t().contiguous()
    wp, fs = torch.tensor([2, 9, 30, 64, 70, 76]), torch.tensor([3.0, -1.5, 0.25, 0.0, -2.0, 20.0])
    wabs = torch.zeros(2, 96); wabs[:, :77] = 1.0
    wsgn = torch.ones(2, 96)
    wabs[1, wp] = fs.abs(); wsgn[1, wp] = fs.sign()
    wabs, wsgn = wabs.to(DEV), wsgn.to(DEV)
    prompt, wset = [1, 0, 1], [-1, 0, 1]
    kw = dict(q_src=list(range(B)), k_src=prompt, v_src=prompt, cross=True, wset=wset, nk_valid=77)
    lib.rt_op_gemm_debug(debug)
    try:
        big, win = out_window(B * N, HD, torch.bfloat16)
        attention(pz(Q), pz(K), pz(VT), B, H, N, 96, DP, wabs=pz(wabs, 0), wsgn=pz(wsgn, 0), O=win, **kw)
        check_windows(f"cross attention N{N} debug {debug:x}", [("O", big, win)])
        plain = attention(Q, K, VT, B, H, N, 96, DP, wabs=wabs, wsgn=wsgn, **kw)
    finally:
        lib.rt_op_gemm_debug(0)
    check_equal(f"cross attention N{N} debug {debug:x}", [("O", win, plain)])
    ref = torch.cat([attn64(Q[b * N:(b + 1) * N], K[prompt[b] * 96:(prompt[b] + 1) * 96], V[prompt[b] * 96:(prompt[b] + 1) * 96], H, DP, 77,
                            wabs[wset[b]] if wset[b] >= 0 else None, wsgn[wset[b]] if wset[b] >= 0 else None) for b in range(B)])
    report(f"cross attention N{N} debug {debug:x}", plain, ref, **ATTN)


@pytest.mark.parametrize("debug", [0, 1 << 19], ids=["runs", "generic"])
def test_attention_keys_memory_contract(debug):
    """Key counts 77, 154 and 231 in ONE launch (cross77_kernel runs plus the tile loop; debug bit 19: the tile loop for all): each prompt's
    rows behind its own key count hold finite junk."""
    lib = _lib()
    B, H, N, DP, P, NK = 3, 2, 64, 64, 3, 288
    HD = H * DP
    counts_p = [77, 154, 231]
    Q, K, V = _cross_inputs(B, H, N, DP, P, NK, counts_p, seed=160)
    VT = V.t().contiguous()
    wpos, fs = torch.tensor([2, 76, 77, 95, 96, 153, 191, 230]), torch.tensor([3.0, -1.5, 0.25, 0.0, -2.0, 20.0, 5.0, -0.5])
    wabs, wsgn = torch.ones(2, NK), torch.ones(2, NK)
    wabs[1, wpos] = fs.abs(); wsgn[1, wpos] = fs.sign()
    wabs, wsgn = wabs.to(DEV), wsgn.to(DEV)
    prompt, wset = [1, 2, 0], [1, 1, -1]
    counts = [counts_p[p] for p in prompt]
    ia = lambda v: (C.c_int * B)(*v)

    def run(Q_, K_, VT_, wabs_, wsgn_, O):
        lib.rt_op_gemm_debug(debug)
        try:
            chk(lib.rt_op_attention_keys(_ptr(Q_), Q_.stride(0), _ptr(K_), K_.stride(0), _ptr(VT_), VT_.stride(0), _ptr(O), O.stride(0), None,
                                         ia(prompt), ia(wset), _ptr(wabs_), _ptr(wsgn_), ia(counts), B, H, N, NK, DP, None))
        finally:
            lib.rt_op_gemm_debug(0)
        torch.cuda.synchronize()
    big, win = out_window(B * N, HD, torch.bfloat16)
    run(pz(Q), pz(K), pz(VT), pz(wabs, 0), pz(wsgn, 0), win)
    check_windows(f"attention_keys debug {debug:x}", [("O", big, win)])
    plain = nans(B * N, HD, torch.bfloat16)
    run(Q, K, VT, wabs, wsgn, plain)
    check_equal(f"attention_keys debug {debug:x}", [("O", win, plain)])
    ref = torch.cat([attn64(Q[b * N:(b + 1) * N], K[prompt[b] * NK:(prompt[b] + 1) * NK], V[prompt[b] * NK:(prompt[b] + 1) * NK], H, DP, counts[b],
                            wabs[wset[b]] if wset[b] >= 0 else None, wsgn[wset[b]] if wset[b] >= 0 else None) for b in range(B)])
    report(f"attention_keys debug {debug:x}", plain, ref, **ATTN)


@pytest.mark.parametrize("B,N,Cc,H", [(2, 128, 1280, 20), (3, 64, 320, 5)])
def test_cross_attn_block_memory_contract(B, N, Cc, H):
    """rt_op_cross_attn_block at the smallest shape of the 1280-channel level (where probe builds fuse to_q and the attention) and one of
    the 320-channel level: trunk_out, q_scratch and o_scratch guarded, every operand between NaN guards, the cached K / V rows 77..95
    finite junk.  Bars: test_cross_attn_block_fused_kernel_against_reference_arithmetic's (O 2e-2, block 3e-2 / 2e-2)."""
    lib = _lib()
    DP = 64
    HD, M, P = H * DP, B * N, 2
    qs = DP ** -0.5 * math.log2(math.e)
    x = bf(rnd(M, Cc, seed=80))
    wq = bf(rnd(HD, Cc, seed=81) * Cc ** -0.5 * qs)
    wo = bf(rnd(Cc, HD, seed=82) * HD ** -0.5)
    bo = (0.1 * rnd(Cc, seed=83)).to(DEV)
    _, K, V = _cross_inputs(1, H, 1, DP, P, 96, [77] * P, seed=84)
    VT = V.t().contiguous()
    wp, fs = torch.tensor([2, 9, 30, 76]), torch.tensor([3.0, -1.5, 0.0, 20.0])
    wabs = torch.zeros(2, 96); wabs[:, :77] = 1.0
    wsgn = torch.ones(2, 96)
    wabs[1, wp] = fs.abs(); wsgn[1, wp] = fs.sign()
    wabs, wsgn = wabs.to(DEV), wsgn.to(DEV)
    prompt = [(b + 1) % P for b in range(B)]
    wset = [1 if b % 2 == 1 else -1 for b in range(B)]
    trunk = (rnd(M, Cc, seed=86) * 2).to(DEV).to(torch.float16)
    ia = lambda v: (C.c_int * B)(*v)

    def run(x_, wq_, wo_, bo_, K_, VT_, wabs_, wsgn_, trunk_, out, q, o):
        chk(lib.rt_op_cross_attn_block(_ptr(x_), _ptr(wq_), _ptr(wo_), _ptr(bo_), _ptr(K_), _ptr(VT_), VT_.stride(0), ia(prompt), ia(wset), _ptr(wabs_),
                                       _ptr(wsgn_), _ptr(trunk_), _ptr(out), _ptr(q), _ptr(o), B, N, Cc, H, DP, None))
        torch.cuda.synchronize()
    name = f"cross_attn_block B{B} N{N} C{Cc}"
    (b1, out_b), (b2, q_b), (b3, o_b) = (guarded((M, c), dt, device=DEV) for c, dt in ((Cc, torch.float16), (HD, torch.bfloat16), (HD, torch.bfloat16)))
    run(pz(x, 0), pz(wq, 0), pz(wo, 0), pz(bo), pz(K, 0), pz(VT), pz(wabs, 0), pz(wsgn, 0), pz(trunk, 0), out_b, q_b, o_b)
    assert intact(b2, q_b), damage(b2, q_b)
    q_written = not bool(torch.isnan(q_b.float()).all())          # probe builds keep Q in LDS at the 1280-channel level: q_scratch is then not written at all
    assert q_written or lib.rt_op_probes_built()
    check_windows(name, [("trunk_out", b1, out_b), ("o_scratch", b3, o_b)] + ([("q_scratch", b2, q_b)] if q_written else []))
    out_a, q_a, o_a = nans(M, Cc, torch.float16), nans(M, HD, torch.bfloat16), nans(M, HD, torch.bfloat16)
    run(x, wq, wo, bo, K, VT, wabs, wsgn, trunk, out_a, q_a, o_a)
    check_equal(name, [("trunk_out", out_b, out_a), ("o_scratch", o_b, o_a)] + ([("q_scratch", q_b, q_a)] if q_written else []))
    qr = (x.double() @ wq.double().t()).to(torch.bfloat16)                     # Q is rounded to bf16 on the way to the attention
    ref_o = torch.cat([attn64(qr[b * N:(b + 1) * N], K[prompt[b] * 96:(prompt[b] + 1) * 96], V[prompt[b] * 96:(prompt[b] + 1) * 96], H, DP, 77,
                              wabs[1] if wset[b] >= 0 else None, wsgn[1] if wset[b] >= 0 else None) for b in range(B)])
    report("cross_attn_block O", o_a, ref_o, atol=2e-2, rtol=2e-2)
    report("cross_attn_block trunk", out_a, ref_o.to(torch.bfloat16).double() @ wo.double().t() + bo.double() + trunk.double(), atol=3e-2, rtol=2e-2)


def test_causal_attention_memory_contract():
    """q, k, v as CLIP's text encoder passes them: three column blocks of ONE buffer (ld = 3 H d + padding), N = 77, ldo > H d."""
    lib = _lib()
    B, H, N, d = 2, 2, 77, 64
    HD = H * d
    qkv = bf(rnd(B * N, 3 * HD, seed=90))
    scale = d ** -0.5

    def run(buf, out):
        es = buf.element_size()
        chk(lib.rt_op_causal_attention(_ptr(buf), C.c_void_p(buf.data_ptr() + HD * es), C.c_void_p(buf.data_ptr() + 2 * HD * es), buf.stride(0),
                                       _ptr(out), out.stride(0), B, H, N, d, C.c_float(scale), None))
        torch.cuda.synchronize()
    big, win = out_window(B * N, HD, torch.bfloat16)
    run(pz(qkv), win)
    check_windows("causal attention", [("out", big, win)])
    plain = nans(B * N, HD, torch.bfloat16)
    run(qkv, plain)
    check_equal("causal attention", [("out", win, plain)])
    v64 = qkv.double().reshape(B, N, 3, H, d).permute(2, 0, 3, 1, 4)          # [3, B, H, N, d]
    s = v64[0] @ v64[1].transpose(-1, -2) * scale
    s = s.masked_fill(torch.ones(N, N, dtype=torch.bool, device=DEV).triu(1), float("-inf"))
    ref = (s.softmax(-1) @ v64[2]).permute(0, 2, 1, 3).reshape(B * N, HD)
    report("causal attention", plain, ref, **ATTN)


# ----------------------------------------------------------------------------------------------- elementwise
@pytest.mark.parametrize("silu_in", [False, True])
@pytest.mark.parametrize("accumulate", [False, True])
def test_small_linear_memory_contract(silu_in, accumulate):
    """B = 7 rows, N = 203 (the last workgroup owns three of its four outputs), K = 72; lda, ldw, ldo padded."""
    B, K, N = 7, 72, 203
    a, W, bias = rnd(B, K, seed=80).to(DEV), bf(rnd(N, K, seed=81, scale=K ** -0.5)), rnd(N, seed=82).to(DEV)
    start = rnd(B, N, seed=83).to(DEV)
    big, win = guarded((B, N), torch.float32, ld=N + 5, device=DEV, fill="bytes" if accumulate else "nan")      # ldo has no multiple to keep
    if accumulate:
        win.copy_(start)
    small_linear(pz(a, K + 4), pz(W), pz(bias), silu_in, out=win, accumulate=accumulate)
    check_windows(f"small_linear silu{silu_in} acc{accumulate}", [("out", big, win)])
    plain = small_linear(a, W, bias, silu_in, out=start.clone() if accumulate else None, accumulate=accumulate)
    check_equal(f"small_linear silu{silu_in} acc{accumulate}", [("out", win, plain)])
    x = a.double()
    ref = (F.silu(x) if silu_in else x) @ W.double().t() + bias.double() + (start.double() if accumulate else 0)
    report(f"small_linear silu{silu_in} acc{accumulate}", plain, ref, atol=1e-4, rtol=1e-4)


@pytest.mark.parametrize("dim", [32, 256, 320])
def test_timestep_embed_memory_contract(dim):
    lib = _lib()
    t = torch.tensor([981.0, 1.0, 500.0, 0.0, 250.5]).to(DEV)
    n = t.numel()

    def run(t_, out):
        chk(lib.rt_op_timestep_embed(_ptr(t_), n, dim, _ptr(out), out.stride(0), None))
        torch.cuda.synchronize()
    big, win = guarded((n, dim), torch.float32, ld=dim + 4, device=DEV)
    run(pz(t), win)
    check_windows(f"timestep_embed {dim}", [("out", big, win)])
    plain = nans(n, dim)
    run(t, plain)
    check_equal(f"timestep_embed {dim}", [("out", win, plain)])
    half = dim // 2
    ang = t.double()[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64, device=DEV) / half)[None, :]
    report(f"timestep_embed {dim}", plain, torch.cat([ang.cos(), ang.sin()], dim=-1), atol=2e-4, rtol=0)        # test_small_linear_and_timestep_embedding's bar


@pytest.mark.parametrize("n", [3 * 1024 - 4, 3 * 1024 + 4, 2048 * 1024 + 4])
def test_cast_bf16_memory_contract(n):
    """One 4-element vector short of / past a multiple of the block's span (256 threads x 4), and one vector past the grid's cap (2048
    blocks: the grid-stride loop's second trip)."""
    lib = _lib()
    x = rnd(n, seed=5).to(DEV)

    def run(x_, out):
        chk(lib.rt_op_cast_bf16(_ptr(x_), _ptr(out), C.c_longlong(n), None))
        torch.cuda.synchronize()
    big, win = guarded((n, 1), torch.bfloat16, device=DEV)                             # a flat vector: rows of one element, guards of 1 MiB
    run(pz(x), win)
    check_windows(f"cast_bf16 {n}", [("out", big, win)])
    plain = nans(n, 1, torch.bfloat16)
    run(x, plain)
    check_equal(f"cast_bf16 {n}", [("out", win, plain)])
    assert torch.equal(plain[:, 0], x.to(torch.bfloat16))                         # round to nearest even: exact


@pytest.mark.parametrize("kind", [0, 1])
@pytest.mark.parametrize("n", [3 * 512 - 2, 3 * 512 + 2, 3 * 512 + 1])
def test_activation_memory_contract(n, kind):
    """One 2-element vector short of / past a multiple of the block's span (256 threads x 2), and an odd count (the last thread owns one element)."""
    lib = _lib()
    x = bf(rnd(n, seed=6) * 2)

    def run(x_, out):
        chk(lib.rt_op_activation(_ptr(x_), _ptr(out), C.c_longlong(n), kind, None))
        torch.cuda.synchronize()
    big, win = guarded((n, 1), torch.bfloat16, device=DEV)
    run(pz(x), win)
    check_windows(f"activation {n} kind {kind}", [("out", big, win)])
    plain = nans(n, 1, torch.bfloat16)
    run(x, plain)
    check_equal(f"activation {n} kind {kind}", [("out", win, plain)])
    v = x.double()
    report(f"activation {n} kind {kind}", plain[:, 0], v * torch.sigmoid(1.702 * v) if kind == 0 else F.gelu(v), **BF16_OUT)


def test_embed_memory_contract():
    """rows = 77 token ids that include 0 and vocab - 1; the id vector sits between out-of-range values (integer poison), the tables between NaN."""
    lib = _lib()
    rows, N, Cc, vocab = 77, 77, 72, 49
    ids = (torch.arange(rows, dtype=torch.int32) * 5) % vocab
    ids[0], ids[-1] = 0, vocab - 1
    ids = ids.to(DEV)
    tok, pos = rnd(vocab, Cc, seed=7).to(DEV), rnd(N, Cc, seed=8).to(DEV)

    def run(ids_, tok_, pos_, out):
        chk(lib.rt_op_embed(_ptr(ids_), _ptr(tok_), _ptr(pos_), _ptr(out), rows, N, Cc, vocab, None))
        torch.cuda.synchronize()
    big, win = guarded((rows, Cc), torch.float32, device=DEV)
    run(pz(ids), pz(tok, 0), pz(pos, 0), win)
    check_windows("embed", [("out", big, win)])
    plain = nans(rows, Cc)
    run(ids, tok, pos, plain)
    check_equal("embed", [("out", win, plain)])
    assert torch.equal(plain, tok[ids.long()] + pos)                           # one fp32 addition: exact
