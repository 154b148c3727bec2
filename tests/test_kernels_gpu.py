"""GPU parity tests of the individual HIP kernels through the C ABI (rt_op_*).

Each kernel is compared with a plain PyTorch fp32 evaluation of the same operator of the reference on
IDENTICAL bf16-rounded inputs, so the tolerances only have to absorb fp32 accumulation order and the final
bf16 rounding of the output (2^-9 relative), not input quantisation.
"""
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hiputil import DEV, attention, bf, gemm, groupnorm, layernorm, report, small_linear, timestep_embed  # noqa: E402

BF16_OUT = dict(atol=2e-2, rtol=1.2e-2)     # bf16 output rounding (0.4 %) + margin, values O(1..10)
F32_OUT = dict(atol=2e-3, rtol=2e-3)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ----------------------------------------------------------------------------------------------- GEMM
@pytest.mark.parametrize("M,N,K", [(128, 128, 64), (256, 384, 128), (448, 320, 320), (1000, 72, 200), (64, 640, 2048),
                                   (4096, 1280, 1280)])
def test_gemm_dense_f32_bias_residual(M, N, K):
    A, W = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2, scale=K ** -0.5))
    bias, res = rnd(N, seed=3).to(DEV), rnd(M, N, seed=4).to(DEV)
    out = gemm(A, W, bias, epi=1, res=res)
    ref = A.float() @ W.float().t() + bias + res
    report(f"gemm_f32 {M}x{N}x{K}", out, ref, **F32_OUT)


@pytest.mark.parametrize("M,N,K", [(256, 128, 64), (1000, 72, 200), (4096, 1280, 1280), (320, 1280, 5120)])
def test_gemm_fp16_trunk_epilogue(M, N, K):
    """epi 4: fp16 output with an fp16 residual, fp32 arithmetic - what every trunk-producing GEMM / conv of the UNet uses."""
    A, W = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2, scale=K ** -0.5))
    bias, res = rnd(N, seed=3).to(DEV), (rnd(M, N, seed=4) * 3).to(DEV).to(torch.float16)
    out = gemm(A, W, bias, epi=4, res=res)
    ref = A.float() @ W.float().t() + bias + res.float()
    assert out.dtype == torch.float16
    report(f"gemm_f16 {M}x{N}x{K}", out, ref, atol=4e-3, rtol=1.5e-3)        # fp16 rounding: 2^-11 relative


def test_gemm_is_transpose_detecting_and_asymmetric():
    # A = I (padded) with asymmetric W catches swapped row/col mapping of the MFMA C layout
    M = N = K = 128
    A = bf(torch.eye(M, K))
    W = bf(torch.arange(N * K, dtype=torch.float32).reshape(N, K) % 251 / 16.0)
    out = gemm(A, W, None, epi=1)
    report("gemm identity", out, W.float().t(), atol=0, rtol=0)


def test_gemm_bf16_out_and_strided_output():
    M, N, K = 320, 192, 256
    A, W = bf(rnd(M, K, seed=5)), bf(rnd(N, K, seed=6, scale=K ** -0.5))
    out = gemm(A, W, None, epi=0)
    report("gemm_bf16", out, A.float() @ W.float().t(), **BF16_OUT)
    # the same problem into a window of a wider buffer (ldo = 232 > N): the same bits, and not a byte outside the window
    from memguard import damage, guarded, intact, unwritten
    big, win = guarded((M, N), torch.bfloat16, ld=232, device=DEV)
    gemm(A, W, None, epi=0, out=win)
    assert intact(big, win), damage(big, win)
    assert unwritten(win) == 0
    assert torch.equal(win, out)


def test_gemm_geglu_epilogue():
    M, C = 256, 64                      # Linear(C, 8C) -> a * gelu(gate)
    A = bf(rnd(M, C, seed=7))
    Wfull = rnd(8 * C, C, seed=8, scale=C ** -0.5)
    bfull = rnd(8 * C, seed=9)
    # engine packing: per 64-row block [32 value rows | 32 gate rows]
    half = 4 * C
    rows = []
    for blk in range(half // 32):
        rows += list(range(blk * 32, blk * 32 + 32)) + list(range(half + blk * 32, half + blk * 32 + 32))
    Wp, bp = bf(Wfull[rows]), bfull[rows].to(DEV).contiguous()
    out = gemm(A, Wp, bp, epi=3)
    h = A.float() @ bf(Wfull).float().t() + bfull.to(DEV)
    a, g = h.chunk(2, dim=-1)
    report("gemm_geglu", out, a * F.gelu(g), **BF16_OUT)


def test_gemm_temb_epilogue():
    B, HW, N, K = 3, 64, 96, 128
    A, W = bf(rnd(B * HW, K, seed=10)), bf(rnd(N, K, seed=11, scale=K ** -0.5))
    bias, temb = rnd(N, seed=12).to(DEV), rnd(B, N, seed=13).to(DEV)
    out = gemm(A, W, bias, epi=2, temb=temb, rows_per_batch=HW)
    ref = (A.float() @ W.float().t() + bias).reshape(B, HW, N) + temb[:, None, :]
    report("gemm_temb", out, ref.reshape(B * HW, N), **BF16_OUT)


@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4, 5, 6, 7, 8])
def test_gemm_tile_configurations_are_bit_identical(cfg):
    """Every tile configuration (incl. the counted-vmcnt rings, the loader-wave, the two-group ping-pong, the 8-phase and the 256x320
    kernels) must give the same bits as cfg 0."""
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    try:
        for (M, N, K) in [(512, 512, 128), (7168, 1280, 1280), (1000, 200, 328), (300, 1280, 64), (2048, 640, 2560), (256, 160, 192), (512, 320, 128), (7168, 1280, 5120)]:
            A, W = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2, scale=K ** -0.5))
            bias, res = rnd(N, seed=3).to(DEV), rnd(M, N, seed=4).to(DEV)
            lib.rt_op_gemm_force_config(0)
            ref = gemm(A, W, bias, epi=1, res=res)
            lib.rt_op_gemm_force_config(cfg)
            for rep in range(3):                      # repeated launches: races show up as run-to-run differences
                out = gemm(A, W, bias, epi=1, res=res)
                assert torch.equal(out, ref), f"cfg {cfg} differs from cfg 0 at {M}x{N}x{K} (rep {rep}): max {(out - ref).abs().max().item()}"
            report(f"gemm cfg{cfg} {M}x{N}x{K}", out, A.float() @ W.float().t() + bias + res, **F32_OUT)
        if cfg == 7:
            return                                    # the 8-phase kernel is dense-only
        # conv through every other configuration
        x = rnd(2, 64, 32, 32, seed=20); w = rnd(96, 64, 3, 3, seed=21, scale=(9 * 64) ** -0.5)
        ref = F.conv2d(x.to(torch.bfloat16).float(), w.to(torch.bfloat16).float(), None, padding=1)
        out = gemm(bf(x.permute(0, 2, 3, 1)), bf(_conv_weight_packed(w)), None, epi=1, mode=1, conv=(32, 32))
        report(f"conv cfg{cfg}", out.reshape(2, 32, 32, 96), ref.permute(0, 2, 3, 1), **F32_OUT)
    finally:
        lib.rt_op_gemm_force_config(-1)


def _gemm16(A, W, bias, epi, variant, res=None, wstat=0, vt=0):
    from rich_text_to_image_amd.engine import load_library, _ptr
    lib = load_library()
    M, K = A.shape
    N = W.shape[0]
    out = torch.empty(M, N // 2 if epi == 3 else N, device=DEV, dtype={1: torch.float32, 4: torch.float16}.get(epi, torch.bfloat16))
    rc = lib.rt_op_gemm16_variant(_ptr(A), _ptr(W), _ptr(bias), _ptr(out), _ptr(res), epi, M, N, K, K, K, out.stride(0),
                                  res.stride(0) if res is not None else 0, vt, variant, wstat, None)
    assert rc == 0, lib.rt_op_last_error().decode()
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("M,N,K", [(7168, 1280, 1280), (5000, 640, 256), (448, 2560, 640), (4096, 1280, 5120),
                                   (7056, 1280, 1280), (28224, 640, 640)])          # 7 streams of SDXL's 96x168 latent: 1008 / 4032 rows each
def test_gemm16_family_classes_and_reference(M, N, K):
    """csrc/gemm16.hip (16x16x32 MFMA, 224-row tiles).  Class A variants (one ascending k sum) must give the bits of gemm.hip's
    32x32x16 kernels and of each other, whatever the tile; class B variants (K split over two waves: even + odd 32-deep k steps)
    must agree with each other bit for bit and with fp32 torch to rounding; all epilogues (bf16, fp32 + residual, fp16 trunk +
    residual) incl. ragged rows."""
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    A, W = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2, scale=K ** -0.5))
    bias = rnd(N, seed=3).to(DEV)
    res32 = rnd(M, N, seed=4).to(DEV)
    res16 = res32.to(torch.float16)
    ref = A.float() @ W.float().t() + bias
    try:
        lib.rt_op_gemm_force_config(0)
        lib.rt_op_gemm_debug(4)                                           # (a small problem would otherwise take gemm.hip's split-K path)
        old = gemm(A, W, bias, epi=1, res=res32)                          # gemm.hip, 128x128 tiles, one ascending k sum
    finally:
        lib.rt_op_gemm_force_config(-1)
        lib.rt_op_gemm_debug(0)
    cls_a = [v for v in (2, 3, 4, 8, 10, 11) if N % {2: 256, 3: 256, 4: 320, 8: 256, 10: 320, 11: 320}[v] == 0]
    for v in cls_a:
        out = _gemm16(A, W, bias, 1, v, res=res32)
        assert torch.equal(out, old), f"class A variant {v} differs from gemm.hip at {M}x{N}x{K}: max {(out - old).abs().max().item()}"
    b0 = _gemm16(A, W, bias, 1, 0, res=res32)
    b1 = _gemm16(A, W, bias, 1, 1, res=res32)
    b9 = _gemm16(A, W, bias, 1, 9, res=res32)
    assert torch.equal(b0, b1) and torch.equal(b0, b9), f"class B variants differ at {M}x{N}x{K}"
    assert torch.equal(_gemm16(A, W, bias, 4, 0, res=res16), _gemm16(A, W, bias, 4, 9, res=res16))
    report(f"gemm16 class B f32+res {M}x{N}x{K}", b0, ref + res32, **F32_OUT)
    report(f"gemm16 class B bf16 {M}x{N}x{K}", _gemm16(A, W, bias, 0, 0), ref, **BF16_OUT)
    report(f"gemm16 class B f16 trunk {M}x{N}x{K}", _gemm16(A, W, bias, 4, 0, res=res16), ref + res16.float(), atol=4e-3, rtol=1.5e-3)
    if cls_a:
        report(f"gemm16 class A f16 trunk {M}x{N}x{K}", _gemm16(A, W, bias, 4, cls_a[0], res=res16), ref + res16.float(), atol=4e-3, rtol=1.5e-3)
    # V^T form (weights on the rows of the output): class B transposed, both column tilings
    if M % 160 == 0 or N % 160 == 0:
        Wv, X = (A, W) if M % 160 == 0 else (W, A)
        t6 = _gemm16(Wv, X, None, 0, 6, vt=1)
        t7 = _gemm16(Wv, X, None, 0, 7, vt=1)
        t12 = _gemm16(Wv, X, None, 0, 12, vt=1)
        assert torch.equal(t6, t7) and torch.equal(t6, t12)
        report("gemm16 V^T", t6, Wv.float() @ X.float().t(), **BF16_OUT)


@pytest.mark.parametrize("streams_qk,streams,rps,C_,HD,expect", [(7, 7, 1024, 1280, 1280, 0), (4, 7, 1024, 1280, 1280, 1), (7, 7, 4096, 640, 640, 0),
                                                                  (4, 7, 4096, 640, 640, 1), (2, 2, 1024, 1280, 1280, 2), (2, 2, 4096, 640, 640, 3),
                                                                  (3, 3, 1024, 1280, 1280, -1), (3, 3, 256, 1280, 1280, -1),
                                                                  # SDXL's 96x168 latent (1008 / 4032 rows per stream): `expect` is whatever
                                                                  # rt_op_gemm_pair_pick answers; grouped or not, both forms face the fp32 reference below
                                                                  (7, 7, 1008, 1280, 1280, None), (4, 7, 1008, 1280, 1280, None),
                                                                  (7, 7, 4032, 640, 640, None), (4, 7, 4032, 640, 640, None)])
def test_grouped_qk_vt_launch_is_bit_identical_with_two_launches(streams_qk, streams, rps, C_, HD, expect):
    """attn1's stacked Q|K projection and V^T = Wv X^T of one LayerNorm output (models/attention_processor.py:495-506) as ONE grouped
    launch (csrc/gemm16.hip, gemm16_dual_kernel): the same tile bodies on one grid, so the bits must equal the two separate launches
    (rt_op_gemm_debug bit 13) at the SDXL shapes of a rich-text step - 7 streams, and 4 streams' Q|K while the region streams are
    injected - and of the 2-stream plain pass; shapes without a grouped form (other batch sizes, small maps) must simply take two launches."""
    import ctypes as C
    from rich_text_to_image_amd.engine import load_library, _ptr
    lib = load_library()
    M, Mqk = streams * rps, streams_qk * rps
    X = bf(rnd(M, C_, seed=1))
    Wqk, Wv = bf(rnd(2 * HD, C_, seed=2, scale=C_ ** -0.5)), bf(rnd(HD, C_, seed=3, scale=C_ ** -0.5))
    bqk = rnd(2 * HD, seed=4).to(DEV)
    pick = lib.rt_op_gemm_pair_pick(streams_qk, streams, rps, 2 * HD, HD, C_)
    print(f"rt_op_gemm_pair_pick({streams_qk}, {streams}, {rps}, {2 * HD}, {HD}, {C_}) = {pick}")
    expect = pick if expect is None else expect
    assert pick == expect

    def run(flags):
        qk = torch.full((M, 2 * HD), 7.0, device=DEV, dtype=torch.bfloat16)          # rows >= Mqk must stay untouched
        vt = torch.zeros(HD, M, device=DEV, dtype=torch.bfloat16)
        grouped = C.c_int(-1)
        lib.rt_op_gemm_debug(flags)
        try:
            rc = lib.rt_op_gemm_qk_vt(_ptr(X), C_, C_, rps, _ptr(Wqk), _ptr(bqk), Mqk, 2 * HD, _ptr(qk), 2 * HD, _ptr(Wv), HD, M, _ptr(vt), M,
                                      C.byref(grouped), None)
        finally:
            lib.rt_op_gemm_debug(0)
        assert rc == 0, lib.rt_op_last_error().decode()
        torch.cuda.synchronize()
        return qk, vt, grouped.value
    qk1, vt1, g1 = run(0)
    qk2, vt2, g2 = run(8192)
    assert g1 == (1 if expect >= 0 else 0) and g2 == 0
    assert torch.equal(qk1, qk2) and torch.equal(vt1, vt2)
    assert bool((qk1[Mqk:] == 7.0).all())
    report(f"grouped Q|K {Mqk}x{2 * HD}x{C_}", qk1[:Mqk], X[:Mqk].float() @ Wqk.float().t() + bqk, **BF16_OUT)
    report(f"grouped V^T {HD}x{M}x{C_}", vt1, Wv.float() @ X.float().t(), **BF16_OUT)
    report(f"two launches Q|K {Mqk}x{2 * HD}x{C_}", qk2[:Mqk], X[:Mqk].float() @ Wqk.float().t() + bqk, **BF16_OUT)
    report(f"two launches V^T {HD}x{M}x{C_}", vt2, Wv.float() @ X.float().t(), **BF16_OUT)


def test_gemm16_geglu_epilogue_and_w_stationary_mapping():
    M, C = 1000, 256
    A = bf(rnd(M, C, seed=7))
    Wfull = rnd(8 * C, C, seed=8, scale=C ** -0.5)
    bfull = rnd(8 * C, seed=9)
    half = 4 * C
    rows = []
    for blk in range(half // 32):
        rows += list(range(blk * 32, blk * 32 + 32)) + list(range(half + blk * 32, half + blk * 32 + 32))
    Wp, bp = bf(Wfull[rows]), bfull[rows].to(DEV).contiguous()
    h = A.float() @ bf(Wfull).float().t() + bfull.to(DEV)
    a, g = h.chunk(2, dim=-1)
    outs = [_gemm16(A, Wp, bp, 3, v, wstat=ws) for v in (2, 3, 8) for ws in (0, 1)]
    for o in outs[1:]:
        assert torch.equal(o, outs[0])                                   # tile shape and tile -> XCD mapping do not change a bit
    report("gemm16 GEGLU", outs[0], a * F.gelu(g), **BF16_OUT)
    assert torch.equal(outs[0], gemm(A, Wp, bp, epi=3))                  # what rt_op_gemm picks (and gemm.hip's GEGLU) agree bit for bit


@pytest.mark.parametrize("B,H,W_,Cin,Cout,epi", [(2, 32, 32, 128, 320, 0), (3, 20, 24, 128, 160, 4), (1, 64, 64, 192, 640, 2), (8, 32, 32, 256, 256, 1),
                                                  (7, 24, 42, 1280, 1280, 4), (2, 48, 84, 640, 640, 4)])      # SDXL 96x168: its /4 and /2 maps, trunk epilogue
def test_conv3x3_on_the_gemm16_main_loop(B, H, W_, Cin, Cout, epi):
    """3x3 stride-1 convolutions with Cin % 64 == 0 run as an implicit GEMM on gemm16.hip's main loop (padding taps read as zeros
    through the buffer descriptor's range check): against F.conv2d, against the patch kernel it replaces (rt_op_gemm_debug(8)),
    for images whose sides are not multiples of 16 as well, with the resnet epilogues (time embedding, fp16 trunk + residual)."""
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    x = rnd(B, Cin, H, W_, seed=20); w = rnd(Cout, Cin, 3, 3, seed=21, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=22).to(DEV)
    ref = F.conv2d(x.to(torch.bfloat16).float().to(DEV), w.to(torch.bfloat16).float().to(DEV), bias, padding=1).permute(0, 2, 3, 1).reshape(B * H * W_, Cout)
    xin, wp = bf(x.permute(0, 2, 3, 1)), bf(_conv_weight_packed(w))
    kw = {}
    if epi == 2:
        temb = rnd(B, Cout, seed=23).to(DEV)
        kw = dict(temb=temb); ref = (ref.reshape(B, H * W_, Cout) + temb[:, None, :]).reshape(B * H * W_, Cout)
    if epi in (1, 4):
        res = rnd(B * H * W_, Cout, seed=24).to(DEV)
        res = res.to(torch.float16) if epi == 4 else res
        kw = dict(res=res); ref = ref + res.float()
    out = gemm(xin, wp, bias, epi=epi, mode=1, conv=(H, W_), **kw)
    tol = {0: BF16_OUT, 2: BF16_OUT, 1: F32_OUT, 4: dict(atol=4e-3, rtol=1.5e-3)}[epi]
    report(f"conv3x3 gemm16 {B}x{H}x{W_}x{Cin}->{Cout} epi{epi}", out, ref, **tol)
    try:
        lib.rt_op_gemm_debug(8)
        old = gemm(xin, wp, bias, epi=epi, mode=1, conv=(H, W_), **kw)
    finally:
        lib.rt_op_gemm_debug(0)
    report("conv3x3 gemm16 vs the kernels it replaces", out, old.float(), **tol)


def test_gemm_repeated_launches_are_bit_identical():
    """(Round 2 ranked tile configurations in situ with HIP events; the choice is now a pure function of the shape.)  48 launches of
    one in-place-residual problem must all give the same bits."""
    M, N, K = 4352, 1280, 704
    A, W = bf(rnd(M, K, seed=1)), bf(rnd(N, K, seed=2, scale=K ** -0.5))
    h0 = rnd(M, N, seed=4).to(DEV)
    from rich_text_to_image_amd.engine import load_library, _ptr
    lib = load_library()
    outs = []
    for _ in range(48):
        h = h0.clone()
        rc = lib.rt_op_gemm(_ptr(A), _ptr(W), None, _ptr(h), _ptr(h), None, 0, 1, M, N, K, K, K, N, N, 0, 0, 0, 0, 0, 0, 0, None)
        assert rc == 0
        outs.append(h)
    torch.cuda.synchronize()
    for h in outs[1:]:
        assert torch.equal(h, outs[0])
    report("in-place residual while the shape is being tuned", outs[0], A.float() @ W.float().t() + h0, **F32_OUT)


def _conv_weight_packed(w):          # [Cout, Cin, 3, 3] -> [Cout, 9*Cin], K = tap*Cin + c
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1)


@pytest.mark.parametrize("mode,B,H,W_,Cin,Cout", [(1, 2, 16, 16, 32, 64), (1, 1, 8, 24, 64, 320), (2, 2, 16, 16, 32, 32),
                                                  (3, 2, 8, 8, 64, 32), (1, 3, 32, 32, 8, 32), (1, 2, 64, 64, 320, 320),
                                                  # the stride-2 down-sampler on maps with h != w at the UNets' widths
                                                  (2, 2, 24, 40, 320, 320), (2, 1, 48, 84, 640, 640), (2, 7, 96, 168, 320, 320)])
def test_conv3x3_implicit_gemm(mode, B, H, W_, Cin, Cout):
    x = rnd(B, Cin, H, W_, seed=20)
    w = rnd(Cout, Cin, 3, 3, seed=21, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=22)
    xb, wb = x.to(torch.bfloat16).float(), w.to(torch.bfloat16).float()
    if mode == 1:
        ref = F.conv2d(xb, wb, bias, padding=1)
    elif mode == 2:
        ref = F.conv2d(xb, wb, bias, stride=2, padding=1)
    else:
        ref = F.conv2d(F.interpolate(xb, scale_factor=2.0, mode="nearest"), wb, bias, padding=1)
    Hout, Wout = ref.shape[2], ref.shape[3]
    A = bf(x.permute(0, 2, 3, 1))                          # NHWC
    out = gemm(A, bf(_conv_weight_packed(w)), bias.to(DEV), epi=1, mode=mode, conv=(Hout, Wout))
    report(f"conv mode{mode} {B}x{H}x{W_}x{Cin}->{Cout}", out.reshape(B, Hout, Wout, Cout), ref.permute(0, 2, 3, 1), **F32_OUT)


@pytest.mark.parametrize("B,H,W_,Cin,Cout,epi", [(2, 32, 32, 64, 96, 1), (1, 16, 48, 128, 200, 1), (3, 16, 16, 192, 160, 0), (2, 32, 16, 64, 320, 2),
                                                  (7, 32, 32, 1280, 1280, 1), (2, 64, 64, 640, 320, 2),
                                                  (1, 64, 64, 128, 128, 1), (1, 32, 32, 256, 256, 1), (2, 16, 32, 64, 512, 0)])   # 128-channel column tiles (VAE widths)
def test_conv3x3_patch_kernel(B, H, W_, Cin, Cout, epi):
    """The 16x16-patch kernel (halo staged once per 64-channel chunk) against torch AND against the implicit-GEMM kernels
    it replaces (same inputs, `rt_op_gemm_debug(1)` routes around it): k order differs, so agreement is to fp32 rounding."""
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    x = rnd(B, Cin, H, W_, seed=20)
    w = rnd(Cout, Cin, 3, 3, seed=21, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=22)
    A, Wp = bf(x.permute(0, 2, 3, 1)), bf(_conv_weight_packed(w))
    res = rnd(B * H * W_, Cout, seed=23).to(DEV) if epi == 1 else None
    temb = rnd(B, Cout, seed=24).to(DEV) if epi == 2 else None
    ref = F.conv2d(x.to(torch.bfloat16).float().to(DEV), w.to(torch.bfloat16).float().to(DEV), bias.to(DEV), padding=1).permute(0, 2, 3, 1)
    if res is not None:
        ref = ref + res.reshape(B, H, W_, Cout)
    if temb is not None:
        ref = ref + temb[:, None, None, :]
    kw = dict(epi=epi, mode=1, conv=(H, W_), res=res, temb=temb)
    try:
        out = gemm(A, Wp, bias.to(DEV), **kw)
        out2 = gemm(A, Wp, bias.to(DEV), **kw)
        assert torch.equal(out, out2), "patch conv is not run-to-run deterministic"
        lib.rt_op_gemm_debug(1)
        old = gemm(A, Wp, bias.to(DEV), **kw)
    finally:
        lib.rt_op_gemm_debug(0)
    tol = F32_OUT if epi == 1 else BF16_OUT
    report(f"patch conv {B}x{H}x{W_}x{Cin}->{Cout} epi{epi} vs torch", out.reshape(B, H, W_, Cout), ref, **tol)
    report("patch conv vs implicit GEMM", out, old, atol=1e-4 if epi == 1 else 2e-2, rtol=1e-4 if epi == 1 else 1e-2)


@pytest.mark.parametrize("H,Cin,Cout,small,big", [(64, 320, 320, 2, 7), (32, 640, 640, 4, 7), (32, 1280, 1280, 5, 7)])
def test_conv3x3_patch_kernel_column_tilings_are_bit_identical(H, Cin, Cout, small, big):
    """The launcher narrows the patch kernel's column tile (160 -> 96 / 64 channels) when a launch would leave CUs idle, so the
    tiling follows the batch size; the k order does not, hence an image must convolve to the same bits alone or in a larger batch
    (64x64x320: 2 images -> 64-channel tiles, 7 -> 160; 32x32x640: 4 -> 64, 7 -> 96; 32x32x1280: 5 -> 64, 7 -> 160)."""
    x = rnd(big, Cin, H, H, seed=30)
    w = rnd(Cout, Cin, 3, 3, seed=31, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=32)
    A, Wp = bf(x.permute(0, 2, 3, 1)), bf(_conv_weight_packed(w))
    full = gemm(A, Wp, bias.to(DEV), epi=0, mode=1, conv=(H, H))
    part = gemm(A[:small].contiguous(), Wp, bias.to(DEV), epi=0, mode=1, conv=(H, H))
    assert torch.equal(full[: small * H * H], part)
    ref = F.conv2d(x[:1].to(torch.bfloat16).float().to(DEV), w.to(torch.bfloat16).float().to(DEV), bias.to(DEV), padding=1).permute(0, 2, 3, 1)
    report(f"patch conv {H}x{H}x{Cin}->{Cout} vs torch", full[: H * H].reshape(1, H, H, Cout), ref, **BF16_OUT)


@pytest.mark.parametrize("mode,B,H,Cin,Cout,epi", [(1, 3, 16, 1280, 1280, 2), (1, 3, 16, 2560, 1280, 4), (1, 4, 16, 1920, 1280, 0), (1, 4, 16, 640, 1280, 1),
                                                   (3, 3, 8, 1280, 1280, 4)])
def test_conv3x3_patch_kernel_split_over_channel_chunks(mode, B, H, Cin, Cout, epi):
    """Round 6: SD-v1.5's 16x16 maps (3 - 5 images of ONE patch each, 640 - 2560 input channels) cannot fill the chip; the patch kernel
    runs them as ~8 slices over the input-channel chunks + the split-K reduction (every epilogue lives there) instead of the split-K
    implicit GEMM (rt_op_gemm_debug bit 28 = the old route).  Against torch, against the old route, run to run, and an image alone
    against the same image in the batch (the slicing is a function of Cin only)."""
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    x = rnd(B, Cin, H, H, seed=40)
    w = rnd(Cout, Cin, 3, 3, seed=41, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=42).to(DEV)
    xb, wb = x.to(torch.bfloat16).float().to(DEV), w.to(torch.bfloat16).float().to(DEV)
    Ho = H if mode == 1 else 2 * H
    ref = F.conv2d(xb if mode == 1 else F.interpolate(xb, scale_factor=2.0, mode="nearest"), wb, bias, padding=1).permute(0, 2, 3, 1).reshape(B * Ho * Ho, Cout)
    kw = {}
    if epi == 2:
        temb = rnd(B, Cout, seed=43).to(DEV)
        kw = dict(temb=temb); ref = (ref.reshape(B, Ho * Ho, Cout) + temb[:, None, :]).reshape(B * Ho * Ho, Cout)
    if epi in (1, 4):
        res = rnd(B * Ho * Ho, Cout, seed=44).to(DEV)
        res = res.to(torch.float16) if epi == 4 else res
        kw = dict(res=res); ref = ref + res.float()
    A, Wp = bf(x.permute(0, 2, 3, 1)), bf(_conv_weight_packed(w))
    try:
        out = gemm(A, Wp, bias, epi=epi, mode=mode, conv=(Ho, Ho), **kw)
        assert torch.equal(out, gemm(A, Wp, bias, epi=epi, mode=mode, conv=(Ho, Ho), **kw)), "not run-to-run deterministic"
        kw1 = {k: (v[:1] if k == "temb" else v[: Ho * Ho]).contiguous() for k, v in kw.items()}
        one = gemm(A[:1].contiguous(), Wp, bias, epi=epi, mode=mode, conv=(Ho, Ho), **kw1)
        assert torch.equal(out[: Ho * Ho], one), "an image alone and in the batch differ"
        lib.rt_op_gemm_debug(1 << 28)
        old = gemm(A, Wp, bias, epi=epi, mode=mode, conv=(Ho, Ho), **kw)
    finally:
        lib.rt_op_gemm_debug(0)
    tol = {0: BF16_OUT, 2: BF16_OUT, 1: F32_OUT, 4: dict(atol=4e-3, rtol=1.5e-3)}[epi]
    report(f"chunk-split patch conv mode{mode} {B}x{H}x{H}x{Cin}->{Cout} epi{epi} vs torch", out, ref, **tol)
    report("chunk-split patch conv vs split-K implicit GEMM", out, old.float(), **tol)


@pytest.mark.parametrize("B,H,W_,Cin,Cout", [(2, 16, 16, 64, 96), (1, 8, 24, 128, 200), (7, 32, 32, 1280, 1280)])
def test_conv3x3_patch_kernel_upsample(B, H, W_, Cin, Cout):
    """Upsample2D folded into the patch kernel (10x10 input halo per 16x16 output patch) vs torch and vs the implicit-GEMM loader."""
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    x = rnd(B, Cin, H, W_, seed=25)
    w = rnd(Cout, Cin, 3, 3, seed=26, scale=(9 * Cin) ** -0.5)
    bias = rnd(Cout, seed=27)
    A, Wp = bf(x.permute(0, 2, 3, 1)), bf(_conv_weight_packed(w))
    xb = x.to(torch.bfloat16).float().to(DEV)
    ref = F.conv2d(F.interpolate(xb, scale_factor=2.0, mode="nearest"), w.to(torch.bfloat16).float().to(DEV), bias.to(DEV), padding=1).permute(0, 2, 3, 1)
    try:
        out = gemm(A, Wp, bias.to(DEV), epi=1, mode=3, conv=(2 * H, 2 * W_))
        lib.rt_op_gemm_debug(1)
        old = gemm(A, Wp, bias.to(DEV), epi=1, mode=3, conv=(2 * H, 2 * W_))
    finally:
        lib.rt_op_gemm_debug(0)
    report(f"patch upsample-conv {B}x{H}x{W_}x{Cin}->{Cout} vs torch", out.reshape(B, 2 * H, 2 * W_, Cout), ref, **F32_OUT)
    report("patch upsample-conv vs implicit GEMM", out, old, atol=1e-4, rtol=1e-4)


# ----------------------------------------------------------------------------------------------- attention
def _ref_attention(q, k, v, heads, fontsize=None):
    """q [B,N,C], k,v [B,NK,C] fp32: the reference math (attention_processor.py:476-545, 359-407)."""
    B, N, Cc = q.shape
    d = Cc // heads

    def h2b(t):
        return t.reshape(B, -1, heads, d).permute(0, 2, 1, 3).reshape(B * heads, -1, d)
    qh, kh, vh = h2b(q), h2b(k), h2b(v)
    s = d ** -0.5 * torch.bmm(qh, kh.transpose(1, 2))
    if fontsize is not None:
        wp, fs = fontsize[0].to(q.device), fontsize[1].to(q.device)
        e = (s - s.max(-1, True)[0]).exp()
        e[:, :, wp] = e[:, :, wp] * fs.abs()
        p = e / e.sum(-1, True)
        p[:, :, wp] *= fs.sign()
    else:
        p = s.softmax(-1)
    o = torch.bmm(p, vh)
    return o.reshape(B, heads, N, d).permute(0, 2, 1, 3).reshape(B, N, Cc), p


def _pack_heads(t, heads, d, DP, scale=1.0):
    """[rows, heads*d] -> bf16 [rows, heads*DP] zero padded"""
    rows = t.shape[0]
    out = torch.zeros(rows, heads, DP)
    out[:, :, :d] = t.reshape(rows, heads, d) * scale
    return bf(out.reshape(rows, heads * DP))


@pytest.mark.parametrize("B,H,N,d", [(2, 2, 256, 64), (1, 4, 128, 8), (2, 3, 320, 40), (1, 2, 64, 160), (1, 2, 192, 80),
                                     (2, 10, 1024, 64),
                                     (3, 2, 144, 64), (2, 5, 400, 64), (2, 2, 16, 32), (1, 3, 72, 40), (2, 2, 1296, 64)])    # ragged: N % 64 != 0
def test_self_attention(B, H, N, d):
    DP = 32 if d <= 32 else 64 if d <= 64 else 96 if d <= 96 else 160
    q, k, v = rnd(B, N, H * d, seed=30), rnd(B, N, H * d, seed=31), rnd(B, N, H * d, seed=32)
    qs = d ** -0.5 * math.log2(math.e)
    Q = _pack_heads(q.reshape(B * N, -1), H, d, DP, qs)
    K = _pack_heads(k.reshape(B * N, -1), H, d, DP)
    V = _pack_heads(v.reshape(B * N, -1), H, d, DP)
    VT = V.t().contiguous()                                     # [H*DP, B*N]
    out = attention(Q, K, VT, B, H, N, N, DP)
    qr = (Q.float() / qs).reshape(B, N, H, DP)[..., :d].reshape(B, N, H * d)
    kr = K.float().reshape(B, N, H, DP)[..., :d].reshape(B, N, H * d)
    vr = V.float().reshape(B, N, H, DP)[..., :d].reshape(B, N, H * d)
    ref, _ = _ref_attention(qr, kr, vr, H)
    got = out.float().reshape(B, N, H, DP)
    assert float(got[..., d:].abs().max()) == 0.0 if DP > d else True
    report(f"self_attn B{B} H{H} N{N} d{d}", got[..., :d].reshape(B, N, H * d), ref, atol=1.5e-2, rtol=1.5e-2)


def test_self_attention_injection_equals_injected_probs():
    """inject(P_ref) == attention with (Q_ref, K_ref, V_region)  (attention_processor.py:522-525)."""
    B, H, N, d, DP = 3, 2, 256, 32, 32
    q, k, v = rnd(B, N, H * d, seed=40), rnd(B, N, H * d, seed=41), rnd(B, N, H * d, seed=42)
    qs = d ** -0.5 * math.log2(math.e)
    Q, K, V = (_pack_heads(t.reshape(B * N, -1), H, d, DP, s) for t, s in ((q, qs), (k, 1.0), (v, 1.0)))
    out = attention(Q, K, V.t().contiguous(), B, H, N, N, DP, q_src=[0, 0, 2], k_src=[0, 0, 2], v_src=[0, 1, 2])
    qr, kr, vr = Q.float().reshape(B, N, -1) / qs, K.float().reshape(B, N, -1), V.float().reshape(B, N, -1)
    _, p_ref = _ref_attention(qr[:1], kr[:1], vr[:1], H)                       # probabilities of stream 0
    vh = vr[1:2].reshape(1, N, H, d).permute(0, 2, 1, 3).reshape(H, N, d)
    inj = torch.bmm(p_ref, vh).reshape(1, H, N, d).permute(0, 2, 1, 3).reshape(N, H * d)
    report("self_attn injected stream", out.float().reshape(B, N, -1)[1], inj, atol=1.5e-2, rtol=1.5e-2)
    own, _ = _ref_attention(qr[2:], kr[2:], vr[2:], H)
    report("self_attn untouched stream", out.float().reshape(B, N, -1)[2], own[0], atol=1.5e-2, rtol=1.5e-2)


@pytest.mark.parametrize("B,H,N,src", [(7, 20, 1024, [0, 1, 2, 3, 3, 3, 3]),        # config 3, injected step, 1280-channel level
                                       (7, 3, 4096, [0, 1, 2, 3, 3, 3, 3]),         # ... 640-channel level (3 of its 10 heads)
                                       (5, 4, 256, [0, 1, 2, 3, 3]),                # R = 2: text_ref + one region
                                       (6, 4, 256, [0, 1, 2, 3, 3, 3]),             # R = 3
                                       (9, 2, 512, [0, 1, 2, 3, 3, 3, 3, 3, 3]),    # R = 6: six members = a unit of four + a unit of two
                                       (6, 2, 320, [0, 0, 2, 3, 3, 3]),             # two shared groups in one launch
                                       (4, 2, 256, [0, 1, 2, 3])])                  # nothing shared: the launch of rounds 1 - 5
def test_self_attention_shared_probability_units_are_bit_identical(B, H, N, src):
    """Round 6: streams that attend with the same (Q, K) source - text_ref and the injected region streams - share ONE softmax per key
    tile (attn_kernel G > 1): per stream the same MFMA sequence, so every mode of launch_attention_units gives the bits of the
    one-stream launches (rt_op_gemm_debug bits 24 - 26: 1 = never, 2 = shared units of G = 4 (or the largest group's 2 / 3) members and the one-stream units in
    ONE launch, 3 = the same with units of two, 4 / 5 = the one-stream units in a launch of their own)."""
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    d = DP = 64
    q, k, v = rnd(B, N, H * d, seed=43), rnd(B, N, H * d, seed=44), rnd(B, N, H * d, seed=45)
    k[:, 5] *= 6.0                                                  # a few dominant keys: the deferred rescale fires in some tiles
    qs = d ** -0.5 * math.log2(math.e)
    Q, K, V = (_pack_heads(t.reshape(B * N, -1), H, d, DP, s) for t, s in ((q, qs), (k, 1.0), (v, 1.0)))
    VT = V.t().contiguous()
    outs = {}
    try:
        for mode in (1, 0, 2, 3, 4, 5):
            lib.rt_op_gemm_debug(mode << 24)
            outs[mode] = attention(Q, K, VT, B, H, N, N, DP, q_src=src, k_src=src, v_src=list(range(B))).clone()
    finally:
        lib.rt_op_gemm_debug(0)
    for mode in (0, 2, 3, 4, 5):
        assert torch.equal(outs[mode], outs[1]), f"mode {mode} differs from the one-stream launches: {(outs[mode].float() - outs[1].float()).abs().max()}"
    # ... and the one-stream launches against the reference arithmetic: stream b = softmax(Q_src K_src^T) V_b
    qr, kr, vr = Q.float().reshape(B, N, -1) / qs, K.float().reshape(B, N, -1), V.float().reshape(B, N, -1)
    b = B - 1
    _, p_ref = _ref_attention(qr[src[b]:src[b] + 1].to(DEV), kr[src[b]:src[b] + 1].to(DEV), vr[:1].to(DEV), H)
    vh = vr[b:b + 1].to(DEV).reshape(1, N, H, d).permute(0, 2, 1, 3).reshape(H, N, d)
    inj = torch.bmm(p_ref, vh).reshape(1, H, N, d).permute(0, 2, 1, 3).reshape(N, H * d)
    report(f"self_attn shared unit, stream {b}", outs[0].float().reshape(B, N, -1)[b], inj, atol=1.5e-2, rtol=1.5e-2)


def test_online_softmax_rescale_branch_with_spiked_keys():
    """Force the running-max rescale: one key per later tile dominates (guide 5.4 rule 26)."""
    B, H, N, d, DP = 1, 1, 256, 64, 64
    q, k, v = rnd(B, N, d, seed=43), rnd(B, N, d, seed=44), rnd(B, N, d, seed=45)
    k[0, 70] = q[0, 5] * 6.0          # spike in tile 1 for query 5
    k[0, 200] = q[0, 5] * 12.0        # bigger spike in tile 3
    k[0, 130] = q[0, 77] * 9.0
    qs = d ** -0.5 * math.log2(math.e)
    Q, K, V = _pack_heads(q[0], H, d, DP, qs), _pack_heads(k[0], H, d, DP), _pack_heads(v[0], H, d, DP)
    out = attention(Q, K, V.t().contiguous(), B, H, N, N, DP)
    ref, _ = _ref_attention(Q.float()[None] / qs, K.float()[None], V.float()[None], H)
    report("self_attn spiked", out.float()[None], ref, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("offset", [-40.0, 40.0])
def test_online_softmax_folded_reference_far_from_zero(offset):
    """The self-attention kernel subtracts its running reference m through an extra MFMA k step (attention.hip FOLD) and keeps m
    bf16-representable.  All scores sit ~290 (log2 domain) below / above zero here - the first tile must re-base from the initial
    reference 0 (exp2 would underflow / overflow otherwise) and m is rounded on a coarse bf16 grid (spacing 2 at 290); later spikes
    force more re-bases.  Softmax is shift invariant, so the fp32 reference is unaffected."""
    B, H, N, d, DP = 2, 2, 512, 64, 64
    q, k, v = rnd(B, N, H * d, seed=46), rnd(B, N, H * d, seed=47), rnd(B, N, H * d, seed=48)
    q, k = q.reshape(B, N, H, d), k.reshape(B, N, H, d)
    q[..., d - 1] = 40.0
    k[..., d - 1] = offset
    k[0, 300, 0, : d - 1] = q[0, 9, 0, : d - 1] * 10.0         # a spike in tile 4 for query 9 of head 0
    q, k = q.reshape(B, N, H * d), k.reshape(B, N, H * d)
    qs = d ** -0.5 * math.log2(math.e)
    Q, K, V = (_pack_heads(t.reshape(B * N, -1), H, d, DP, s) for t, s in ((q, qs), (k, 1.0), (v, 1.0)))
    out = attention(Q, K, V.t().contiguous(), B, H, N, N, DP)
    ref, _ = _ref_attention(Q.float().reshape(B, N, -1) / qs, K.float().reshape(B, N, -1), V.float().reshape(B, N, -1), H)
    assert torch.isfinite(out.float()).all()
    report(f"self_attn scores offset {offset:+.0f}", out.float().reshape(B, N, -1), ref, atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("use_fs", [False, True])
def test_cross_attention_fontsize(use_fs):
    B, H, N, d, DP, P = 3, 2, 256, 32, 32, 2
    q = rnd(B, N, H * d, seed=50)
    kc, vc = rnd(P, 77, H * d, seed=51), rnd(P, 77, H * d, seed=52)
    qs = d ** -0.5 * math.log2(math.e)
    Q = _pack_heads(q.reshape(B * N, -1), H, d, DP, qs)
    Kp = torch.zeros(P, 96, H * d); Kp[:, :77] = kc
    Vp = torch.zeros(P, 96, H * d); Vp[:, :77] = vc
    K = _pack_heads(Kp.reshape(P * 96, -1), H, d, DP)
    V = _pack_heads(Vp.reshape(P * 96, -1), H, d, DP)
    wp, fs = torch.tensor([2, 9, 30]), torch.tensor([3.0, -1.5, 0.25])
    wabs = torch.zeros(2, 96); wabs[:, :77] = 1.0
    wsgn = torch.ones(2, 96)
    wabs[1, wp] = fs.abs(); wsgn[1, wp] = fs.sign()
    prompt = [0, 1, 1]
    wset = [0, 1 if use_fs else 0, 0]
    out = attention(Q, K, V.t().contiguous(), B, H, N, 96, DP, q_src=[0, 1, 2], k_src=prompt, v_src=prompt, cross=True,
                    wabs=wabs.to(DEV), wsgn=wsgn.to(DEV), wset=wset, nk_valid=77)
    qr = Q.float().reshape(B, N, -1) / qs
    kr = K.float().reshape(P, 96, -1)[:, :77]
    vr = V.float().reshape(P, 96, -1)[:, :77]
    for b in range(B):
        ref, _ = _ref_attention(qr[b:b + 1], kr[prompt[b]][None], vr[prompt[b]][None], H, (wp, fs) if wset[b] else None)
        report(f"cross_attn stream {b} fs={wset[b]}", out.float().reshape(B, N, -1)[b], ref[0], atol=1.5e-2, rtol=1.5e-2)


@pytest.mark.parametrize("B,H,N", [(3, 4, 256), (7, 20, 1024), (2, 10, 4096), (2, 5, 320)])
def test_cross77_kernel_against_reference_arithmetic_and_the_generic_kernel(B, H, N):
    """cross77_kernel (csrc/cross77.hip: what the engine runs for attn2 at d = 64 - 64 queries x 2 heads per workgroup, K / V^T of the
    cached 77 keys in LDS, key mask and |font size| as an additive log2 bias on the scores) through rt_op_attention: against the
    reference processor's arithmetic in fp32 (attention_processor.py:476-545, font-size softmax :386-401) with a NEGATIVE size, a ZERO
    size, the last valid key (76) and junk in the padded V rows, streams mixing prompts and plain / font-size softmax - and against
    the generic attn_kernel<CROSS> on the same inputs (debug bit 19)."""
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    d = DP = 64
    P = 3
    q = rnd(B, N, H * d, seed=60) * 3.0                                       # scores of a few units: a peaked softmax
    kc, vc = rnd(P, 77, H * d, seed=61), rnd(P, 77, H * d, seed=62)
    qs = d ** -0.5 * math.log2(math.e)
    Q = _pack_heads(q.reshape(B * N, -1), H, d, DP, qs)
    Kp = torch.zeros(P, 96, H * d); Kp[:, :77] = kc
    Vp = torch.full((P, 96, H * d), 7.0); Vp[:, :77] = vc                      # padded keys carry junk values: they must be masked, not multiplied by ~0
    K = _pack_heads(Kp.reshape(P * 96, -1), H, d, DP)
    V = _pack_heads(Vp.reshape(P * 96, -1), H, d, DP)
    wp, fs = torch.tensor([2, 9, 30, 64, 70, 76]), torch.tensor([3.0, -1.5, 0.25, 0.0, -2.0, 20.0])
    wabs = torch.zeros(2, 96); wabs[:, :77] = 1.0
    wsgn = torch.ones(2, 96)
    wabs[1, wp] = fs.abs(); wsgn[1, wp] = fs.sign()
    prompt = [(2 * b + 1) % P for b in range(B)]
    wset = [1 if b % 3 == 1 else -1 for b in range(B)]
    kw = dict(q_src=list(range(B)), k_src=prompt, v_src=prompt, cross=True, wabs=wabs.to(DEV), wsgn=wsgn.to(DEV), wset=wset, nk_valid=77)
    out = attention(Q, K, V.t().contiguous(), B, H, N, 96, DP, **kw)
    lib.rt_op_gemm_debug(524288)
    try:
        generic = attention(Q, K, V.t().contiguous(), B, H, N, 96, DP, **kw)
    finally:
        lib.rt_op_gemm_debug(0)
    assert torch.isfinite(out.float()).all()
    qr = Q.float().reshape(B, N, -1) / qs
    kr, vr = K.float().reshape(P, 96, -1)[:, :77], V.float().reshape(P, 96, -1)[:, :77]
    for b in range(min(B, 4)):
        ref, _ = _ref_attention(qr[b:b + 1], kr[prompt[b]][None], vr[prompt[b]][None], H, (wp, fs) if wset[b] >= 0 else None)
        report(f"cross77 B{B} H{H} N{N} stream {b} fs={wset[b]}", out.float().reshape(B, N, -1)[b], ref[0], atol=2e-2, rtol=2e-2)
    report("cross77 vs attn_kernel<CROSS>", out.float(), generic.float(), atol=2e-2, rtol=2e-2)
    # its tiling choices (heads per workgroup, query tiles per wave: debug bits 21 / 20) never change a query's arithmetic
    for bits in (1048576, 2097152, 3145728):
        lib.rt_op_gemm_debug(bits)
        try:
            other = attention(Q, K, V.t().contiguous(), B, H, N, 96, DP, **kw)
        finally:
            lib.rt_op_gemm_debug(0)
        assert torch.equal(other, out), bits


def test_cross_attention_plain_path_equals_the_tables_of_ones():
    """wset[b] < 0 selects plain softmax over the nk_valid keys without multiplier tables (attention.hip: what the engine passes for
    every stream without a font-size entry).  It must agree BIT FOR BIT with wset = 0 on tables of ones / zeros for the padded keys:
    multiplying by 1.0 and by the 0 of a key whose score was masked to -inf changes nothing - in a batch that mixes both kinds."""
    B, H, N, d, DP, P = 4, 3, 384, 64, 64, 2
    q = rnd(B, N, H * d, seed=53)
    kc, vc = rnd(P, 77, H * d, seed=54), rnd(P, 77, H * d, seed=55)
    qs = d ** -0.5 * math.log2(math.e)
    Q = _pack_heads(q.reshape(B * N, -1), H, d, DP, qs)
    Kp = torch.zeros(P, 96, H * d); Kp[:, :77] = kc
    Vp = torch.zeros(P, 96, H * d); Vp[:, :77] = vc
    K, V = _pack_heads(Kp.reshape(P * 96, -1), H, d, DP), _pack_heads(Vp.reshape(P * 96, -1), H, d, DP)
    wp, fs = torch.tensor([4, 11]), torch.tensor([2.5, -0.75])
    wabs = torch.zeros(2, 96); wabs[:, :77] = 1.0
    wsgn = torch.ones(2, 96)
    wabs[1, wp] = fs.abs(); wsgn[1, wp] = fs.sign()
    prompt = [0, 1, 1, 0]
    kw = dict(q_src=[0, 1, 2, 3], k_src=prompt, v_src=prompt, cross=True, wabs=wabs.to(DEV), wsgn=wsgn.to(DEV), nk_valid=77)
    tables = attention(Q, K, V.t().contiguous(), B, H, N, 96, DP, wset=[0, 1, 0, 0], **kw)
    plain = attention(Q, K, V.t().contiguous(), B, H, N, 96, DP, wset=[-1, 1, -1, -1], **kw)
    assert torch.equal(tables, plain)
    qr = Q.float().reshape(B, N, -1) / qs
    kr, vr = K.float().reshape(P, 96, -1)[:, :77], V.float().reshape(P, 96, -1)[:, :77]
    for b in (0, 1):
        ref, _ = _ref_attention(qr[b:b + 1], kr[prompt[b]][None], vr[prompt[b]][None], H, (wp, fs) if b == 1 else None)
        report(f"cross_attn plain-path batch, stream {b}", plain.float().reshape(B, N, -1)[b], ref[0], atol=1.5e-2, rtol=1.5e-2)


def test_attention_against_reference_module_golden():
    """tests/golden/attention_ops.pt was produced by the UNMODIFIED reference Attention module."""
    import os
    g = torch.load(os.path.join(os.path.dirname(__file__), "golden", "attention_ops.pt"))
    H, d, DP = 2, 32, 32
    qs = d ** -0.5 * math.log2(math.e)
    x, ctx = g["x"], g["ctx"]
    B, N, Cc = x.shape
    sd = g["cross_sd"]
    q = F.linear(x, sd["to_q.weight"]); k = F.linear(ctx, sd["to_k.weight"]); v = F.linear(ctx, sd["to_v.weight"])
    Q = _pack_heads(q.reshape(B * N, -1), H, d, DP, qs)
    Kp = torch.zeros(B, 96, H * d); Kp[:, :77] = k
    Vp = torch.zeros(B, 96, H * d); Vp[:, :77] = v
    K = _pack_heads(Kp.reshape(B * 96, -1), H, d, DP); V = _pack_heads(Vp.reshape(B * 96, -1), H, d, DP)
    wabs = torch.zeros(2, 96); wabs[:, :77] = 1.0
    wsgn = torch.ones(2, 96)
    wabs[1, g["word_pos"]] = g["font_size"].abs(); wsgn[1, g["word_pos"]] = g["font_size"].sign()
    for name, ws in (("y_plain", [0, 0]), ("y_fs", [1, 1])):
        o = attention(Q, K, V.t().contiguous(), B, H, N, 96, DP, k_src=[0, 1], v_src=[0, 1], cross=True, wabs=wabs.to(DEV),
                      wsgn=wsgn.to(DEV), wset=ws, nk_valid=77)
        y = F.linear(o.float().cpu(), sd["to_out.0.weight"], sd["to_out.0.bias"]).reshape(B, N, Cc)
        report(f"reference Attention module {name}", y, g[name], atol=3e-2, rtol=3e-2)
    # self attention + injection
    sd = g["self_sd"]
    q, k, v = (F.linear(x, sd[f"to_{n}.weight"]) for n in "qkv")
    v2 = F.linear(g["x2"], sd["to_v.weight"])
    Q = _pack_heads(torch.cat([q, q]).reshape(2 * B * N, -1), H, d, DP, qs)
    K = _pack_heads(torch.cat([k, k]).reshape(2 * B * N, -1), H, d, DP)
    V = _pack_heads(torch.cat([v, v2]).reshape(2 * B * N, -1), H, d, DP)
    o = attention(Q, K, V.t().contiguous(), 2 * B, H, N, N, DP, q_src=[0, 1, 0, 1], k_src=[0, 1, 0, 1], v_src=[0, 1, 2, 3])
    y = F.linear(o.float().cpu(), sd["to_out.0.weight"], sd["to_out.0.bias"]).reshape(2 * B, N, Cc)
    report("reference Attention module y_self", y[:B], g["y_self"], atol=3e-2, rtol=3e-2)
    report("reference Attention module y_inj (real_attn_probs)", y[B:], g["y_inj"], atol=3e-2, rtol=3e-2)


def test_cross_attn_block_op_against_reference_module_golden():
    """rt_op_cross_attn_block = to_q -> attention over the cached 77 keys (font-size softmax) -> to_out + bias + fp16 trunk residual in
    one C-ABI call, against the outputs of the UNMODIFIED reference Attention module (golden y_plain / y_fs incl. a negative font
    size) plus the residual the BasicTransformerBlock adds around it (attention.py:169-189)."""
    import ctypes as C
    import os
    from rich_text_to_image_amd.engine import load_library, _ptr
    g = torch.load(os.path.join(os.path.dirname(__file__), "golden", "attention_ops.pt"))
    lib = load_library()
    H, d, DP = 2, 32, 32
    qs = d ** -0.5 * math.log2(math.e)
    x, ctx, sd = g["x"], g["ctx"], g["cross_sd"]
    B, N, Cc = x.shape
    assert (g["font_size"] < 0).any()
    k = F.linear(ctx, sd["to_k.weight"]); v = F.linear(ctx, sd["to_v.weight"])
    Kp = torch.zeros(B, 96, H * d); Kp[:, :77] = k
    Vp = torch.zeros(B, 96, H * d); Vp[:, :77] = v
    K = _pack_heads(Kp.reshape(B * 96, -1), H, d, DP); VT = _pack_heads(Vp.reshape(B * 96, -1), H, d, DP).t().contiguous()
    wq = _pack_heads(sd["to_q.weight"].t().contiguous(), H, d, DP, qs).t().contiguous()          # [H*DP, C], pre-scaled
    wo = torch.zeros(Cc, H * DP); wo.reshape(Cc, H, DP)[:, :, :d] = sd["to_out.0.weight"].reshape(Cc, H, d)
    wo, bo = bf(wo), sd["to_out.0.bias"].float().to(DEV).contiguous()
    wabs = torch.zeros(2, 96); wabs[:, :77] = 1.0
    wsgn = torch.ones(2, 96)
    wabs[1, g["word_pos"]] = g["font_size"].abs(); wsgn[1, g["word_pos"]] = g["font_size"].sign()
    wabs, wsgn = wabs.to(DEV), wsgn.to(DEV)
    xb = bf(x.reshape(B * N, Cc))
    trunk = (rnd(B * N, Cc, seed=5) * 2).to(DEV).to(torch.float16).contiguous()
    q = torch.empty(B * N, H * DP, device=DEV, dtype=torch.bfloat16); o = torch.empty_like(q)
    ia = lambda vals: (C.c_int * B)(*vals)
    for name, ws in (("y_plain", [0, 0]), ("y_fs", [1, 1])):
        out = torch.empty_like(trunk)
        rc = lib.rt_op_cross_attn_block(_ptr(xb), _ptr(wq), _ptr(wo), _ptr(bo), _ptr(K), _ptr(VT), VT.stride(0), ia([0, 1]), ia(ws), _ptr(wabs),
                                        _ptr(wsgn), _ptr(trunk), _ptr(out), _ptr(q), _ptr(o), B, N, Cc, H, DP, None)
        assert rc == 0, lib.rt_op_last_error().decode()
        torch.cuda.synchronize()
        report(f"rt_op_cross_attn_block {name}", out.float().cpu(), g[name].reshape(B * N, Cc) + trunk.float().cpu(), atol=3e-2, rtol=3e-2)


@pytest.mark.parametrize("B,N,Cc,H", [(3, 256, 320, 5), (7, 1024, 1280, 20), (2, 384, 640, 10), (3, 1024, 640, 10)])
def test_cross_attn_block_fused_kernel_against_reference_arithmetic(B, N, Cc, H):
    """rt_op_cross_attn_block in all of its forms - the engine's (to_q GEMM -> cross77_kernel -> to_out GEMM, round 5), round 4's fused
    to_q + 77-key attention kernel (csrc/gemm16.hip, EPI_XATTN; debug bit 19), the generic three launches (bits 4 + 19) and, at 640
    channels, the one-launch xblock kernel (bit 16) - on shapes that take them (d = 64, H % 5 == 0, N % 128 == 0): against the reference processor's
    arithmetic in fp32 (attention_processor.py:476-545, font-size softmax :386-401 incl. a NEGATIVE size; attention.py:169-189 adds
    the residual) on identical bf16-rounded operands, and against the three-launch form of the same operator (debug bit 4).
    Streams mix prompts and plain / font-size softmax, so a tile's K / V^T and multiplier set follow ITS stream."""
    import ctypes as C
    from rich_text_to_image_amd.engine import load_library, _ptr
    lib = load_library()
    d = DP = 64
    P = 3
    qs = d ** -0.5 * math.log2(math.e)
    x = bf(rnd(B * N, Cc, seed=80))
    wq_f = rnd(H * d, Cc, seed=81) * Cc ** -0.5 * 3.0                       # scores of a few units: a peaked softmax
    wq = bf(wq_f * qs)
    wo = bf(rnd(Cc, H * d, seed=82) * (H * d) ** -0.5)
    bo = (0.1 * rnd(Cc, seed=83)).to(DEV).contiguous()
    kc, vc = rnd(P, 77, H * d, seed=84), rnd(P, 77, H * d, seed=85)
    Kp = torch.zeros(P, 96, H * d); Kp[:, :77] = kc
    Vp = torch.full((P, 96, H * d), 7.0); Vp[:, :77] = vc                    # padded keys carry junk values: they must be masked, not multiplied by ~0
    K = bf(Kp.reshape(P * 96, -1)); VT = bf(Vp.reshape(P * 96, -1)).t().contiguous()
    wp, fs = torch.tensor([2, 9, 30, 76]), torch.tensor([3.0, -1.5, 0.25, 20.0])
    wabs = torch.zeros(2, 96); wabs[:, :77] = 1.0
    wsgn = torch.ones(2, 96)
    wabs[1, wp] = fs.abs(); wsgn[1, wp] = fs.sign()
    wabs, wsgn = wabs.to(DEV), wsgn.to(DEV)
    prompt = [(2 * b + 1) % P for b in range(B)]
    wset = [1 if b % 3 == 1 else -1 for b in range(B)]
    trunk = (rnd(B * N, Cc, seed=86) * 2).to(DEV).to(torch.float16).contiguous()
    ia = lambda vals: (C.c_int * B)(*vals)

    def run():
        q = torch.zeros(B * N, H * DP, device=DEV, dtype=torch.bfloat16); o = torch.zeros_like(q); out = torch.empty_like(trunk)
        rc = lib.rt_op_cross_attn_block(_ptr(x), _ptr(wq), _ptr(wo), _ptr(bo), _ptr(K), _ptr(VT), VT.stride(0), ia(prompt), ia(wset), _ptr(wabs),
                                        _ptr(wsgn), _ptr(trunk), _ptr(out), _ptr(q), _ptr(o), B, N, Cc, H, DP, None)
        assert rc == 0, lib.rt_op_last_error().decode()
        torch.cuda.synchronize()
        return out.float().cpu(), o.float().cpu(), q
    # shapes of the 640-channel level can take xblock.hip (the whole block in ONE launch: neither Q nor O reaches HBM) - opt-in through
    # debug bit 16, because it measured slower than the separate launches (LABNOTES R5.2); its arithmetic stays pinned here
    # (both probe kernels live in `make PROBES=1` builds only since round 6: rt_op_probes_built(); the shipped library runs the engine's form
    #  and the generic three launches)
    probes = bool(lib.rt_op_probes_built())
    is_xblock = probes and Cc == 640 and H == 10 and N % 128 == 0
    if is_xblock:
        lib.rt_op_gemm_debug(65536)
        try:
            block, o_block, q_block = run()
        finally:
            lib.rt_op_gemm_debug(0)
        assert float(q_block.float().abs().max()) == 0.0 and float(o_block.float().abs().max()) == 0.0, "xblock must write neither Q nor O"
    # the engine's form (round 5): to_q GEMM -> cross77_kernel -> to_out GEMM
    engine_form, o_engine, q_engine = run()
    if N % 64 == 0:                                                        # cross77's shapes (d = 64, whole 64-query blocks)
        assert float(q_engine.float().abs().max()) > 0.0
    fused = o_fused = None
    if probes:
        lib.rt_op_gemm_debug(524288)                                       # bit 19: round 4's forms - EPI_XATTN where the tiling allows it
        try:
            fused, o_fused, q_fused = run()
        finally:
            lib.rt_op_gemm_debug(0)
        assert float(q_fused.float().abs().max()) == 0.0, "the fused path must not write Q to HBM"
    lib.rt_op_gemm_debug(16 | 524288)                                      # to_q GEMM -> attn_kernel<CROSS> -> to_out GEMM
    try:
        three, o_three, q_three = run()
    finally:
        lib.rt_op_gemm_debug(0)
    assert float(q_three.float().abs().max()) > 0.0
    # fp32 reference on the same bf16-rounded operands; Q rounded to bf16 like both device paths do
    xq = (x.float().cpu() @ wq.float().cpu().t()).to(torch.bfloat16).float() / qs
    kr, vr = K.float().cpu().reshape(P, 96, -1)[:, :77], VT.float().cpu().t().reshape(P, 96, -1)[:, :77]
    ref_o = torch.empty(B, N, H * d)
    for b in range(B):
        ref_o[b], _ = _ref_attention(xq.reshape(B, N, -1)[b:b + 1], kr[prompt[b]][None], vr[prompt[b]][None], H, (wp, fs) if wset[b] >= 0 else None)
    ref = ref_o.reshape(B * N, -1).to(torch.bfloat16).float() @ wo.float().cpu().t() + bo.cpu() + trunk.float().cpu()
    if probes:
        report(f"fused attention output O B{B} N{N} C{Cc}", o_fused, ref_o.reshape(B * N, -1), atol=2e-2, rtol=2e-2)
        report(f"rt_op_cross_attn_block fused B{B} N{N} C{Cc}", fused, ref, atol=3e-2, rtol=2e-2)
        report("fused vs three-launch form", fused, three, atol=3e-2, rtol=2e-2)
        report("fused O vs three-launch O", o_fused, o_three, atol=2e-2, rtol=2e-2)
    report(f"three-launch form O B{B} N{N} C{Cc}", o_three, ref_o.reshape(B * N, -1), atol=2e-2, rtol=2e-2)
    report("engine form vs three-launch form", engine_form, three, atol=3e-2, rtol=2e-2)
    report(f"engine form (to_q -> cross77 -> to_out) O B{B} N{N} C{Cc}", o_engine, ref_o.reshape(B * N, -1), atol=2e-2, rtol=2e-2)
    report(f"rt_op_cross_attn_block engine form B{B} N{N} C{Cc}", engine_form, ref, atol=3e-2, rtol=2e-2)
    if is_xblock:
        report(f"xblock (one launch) B{B} N{N} C{Cc}", block, ref, atol=3e-2, rtol=2e-2)
        report("xblock vs three-launch form", block, three, atol=3e-2, rtol=2e-2)


# ----------------------------------------------------------------------------------------------- norms
# The launch form (csrc/norm.hip gn_fused_vw through the host query: 1 = one launch, 2 = two launches) of test_groupnorm's cases whose HW is
# not a power of two, keyed (HW, C1, C2): HW 1008 (40 and 80 channels per group), 96 (80) and 384 (60: 4-wide loads) take the ONE-launch
# form, HW 4032 and the fp32-input 16128 the two-launch form.  A change of the rule fails the assertion instead of silently moving a case.
GN_FORM_NOT_POW2 = {(1008, 1280, 0): 1, (1008, 1280, 1280): 1, (4032, 640, 640): 2, (96, 1280, 1280): 1, (384, 1280, 640): 1, (16128, 320, 0): 2}


@pytest.mark.parametrize("B,HW,C1,C2,G,silu,bf16in", [(2, 256, 64, 0, 8, True, False), (3, 1024, 320, 0, 32, True, False),
                                                      (2, 64, 1280, 640, 32, True, False), (2, 4096, 640, 320, 32, True, False),
                                                      (2, 256, 320, 0, 32, False, False), (2, 1024, 96, 0, 8, True, True),
                                                      (1, 16384, 320, 0, 32, True, False),
                                                      (2, 64, 1280, 640, 32, True, "f16"), (2, 1024, 320, 0, 32, False, "f16"),
                                                      (3, 256, 96, 32, 8, True, "f16"),
                                                      # the one-launch form at the UNets' own shapes (SD-v1.5 16^2 / 32^2, SDXL 32^2 / 64^2)
                                                      (3, 256, 1280, 1280, 32, True, "f16"), (7, 1024, 1280, 0, 32, False, "f16"),
                                                      (2, 4096, 640, 0, 32, True, "f16"), (3, 1024, 640, 640, 32, True, "f16"),
                                                      (2, 1024, 1280, 640, 32, True, "f16"),
                                                      # HW that are not powers of two: the maps of SDXL 96x168 (1008 / 4032 / 16128) and SD-v1.5 64x96 (96 / 384);
                                                      # the form each of them takes is asserted through rt_op_groupnorm_form (GN_FORM_NOT_POW2 below)
                                                      (7, 1008, 1280, 0, 32, True, "f16"), (7, 1008, 1280, 1280, 32, True, "f16"),
                                                      (2, 4032, 640, 640, 32, True, "f16"), (3, 96, 1280, 1280, 32, True, "f16"),
                                                      (3, 384, 1280, 640, 32, True, "f16"), (1, 16128, 320, 0, 32, True, False)])
def test_groupnorm(B, HW, C1, C2, G, silu, bf16in):
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    if (HW, C1, C2) in GN_FORM_NOT_POW2:
        in_type = 2 if bf16in == "f16" else 1 if bf16in else 0
        assert lib.rt_op_groupnorm_form(in_type, C1, C2, G, B, HW) == GN_FORM_NOT_POW2[(HW, C1, C2)], (HW, C1, C2)
    x1 = rnd(B, HW, C1, seed=60) * 2 + 0.5
    x2 = rnd(B, HW, C2, seed=61) - 0.3 if C2 else None
    gamma, beta = (1 + 0.1 * rnd(C1 + C2, seed=62)).to(DEV), (0.1 * rnd(C1 + C2, seed=63)).to(DEV)
    eps = 1e-5 if silu else 1e-6
    if bf16in == "f16":                              # fp16 trunk tensors incl. the virtual concat of the up blocks
        x1 = x1.to(torch.float16)
        x2 = x2.to(torch.float16) if C2 else None
    elif bf16in:
        x1 = x1.to(torch.bfloat16)
    xin1 = x1.to(DEV).contiguous()
    xin2 = x2.to(DEV).contiguous() if C2 else None
    out, raw = groupnorm(xin1, xin2, G, gamma, beta, eps, silu, want_raw=True)
    xc = torch.cat([x1.float(), x2.float()], -1) if C2 else x1.float()
    ref = F.group_norm(xc.permute(0, 2, 1).to(DEV), G, gamma, beta, eps).permute(0, 2, 1)
    if silu:
        ref = F.silu(ref)
    report(f"groupnorm B{B} HW{HW} C{C1}+{C2}", out, ref, **BF16_OUT)
    report("groupnorm raw copy", raw, xc, atol=1e-2, rtol=8e-3)
    # round 6: shapes where one workgroup owns a whole (batch entry, group) run as ONE launch; rt_op_gemm_debug bit 23 = the two-launch
    # form.  Same statistics to fp32 rounding, and an image alone equals the same image in the batch in either form.
    try:
        lib.rt_op_gemm_debug(1 << 23)
        two = groupnorm(xin1, xin2, G, gamma, beta, eps, silu)
    finally:
        lib.rt_op_gemm_debug(0)
    report("groupnorm one launch vs two launches", out, two.float(), atol=2e-2, rtol=8e-3)
    one = groupnorm(xin1[:1].contiguous(), xin2[:1].contiguous() if C2 else None, G, gamma, beta, eps, silu)
    assert torch.equal(one, out[:1]), "an image alone and in the batch differ"


@pytest.mark.parametrize("f16", [False, True])
@pytest.mark.parametrize("rows,C", [(100, 64), (512, 640), (1024, 1280), (77, 320), (1021, 640), (515, 1280), (96, 768)])
def test_layernorm(rows, C, f16):
    x = (rnd(rows, C, seed=70) * 3 + 1).to(DEV)
    if f16:
        x = x.to(torch.float16)                     # the UNet trunk is fp16; the text encoder's residual stream fp32
    gamma, beta = (1 + 0.1 * rnd(C, seed=71)).to(DEV), (0.1 * rnd(C, seed=72)).to(DEV)
    out = layernorm(x, gamma, beta)
    report(f"layernorm {rows}x{C}", out, F.layer_norm(x.float(), (C,), gamma, beta, 1e-5), **BF16_OUT)


def test_small_linear_and_timestep_embedding():
    B, K, N = 7, 320, 1280
    a, W, bias = rnd(B, K, seed=80).to(DEV), bf(rnd(N, K, seed=81, scale=K ** -0.5)), rnd(N, seed=82).to(DEV)
    report("small_linear", small_linear(a, W, bias), a @ W.float().t() + bias, atol=1e-4, rtol=1e-4)
    report("small_linear silu", small_linear(a, W, bias, True), F.silu(a) @ W.float().t() + bias, atol=1e-4, rtol=1e-4)
    from oracle.unet import timestep_embedding
    t = torch.tensor([981.0, 1.0, 500.0, 1024.0, 0.0])
    for dim in (320, 256, 32):
        report(f"timestep_embed {dim}", timestep_embed(t.to(DEV), dim), timestep_embedding(t, dim), atol=2e-4, rtol=0)


# ----------------------------------------------------------------------------------------------- AttnProcessor seam
class _StubAttention:
    """The attributes of the reference `Attention` module the processor contract reads (attention_processor.py:33-152)."""

    def __init__(self, sd, heads, cross_dim=None):
        import torch.nn as nn
        inner, qdim = sd["to_q.weight"].shape
        self.heads, self.scale = heads, (inner // heads) ** -0.5
        self.to_q = nn.Linear(qdim, inner, bias=False); self.to_k = nn.Linear(cross_dim or qdim, inner, bias=False)
        self.to_v = nn.Linear(cross_dim or qdim, inner, bias=False)
        self.to_out = nn.ModuleList([nn.Linear(inner, qdim), nn.Dropout(0.0)])
        for n, m in (("to_q", self.to_q), ("to_k", self.to_k), ("to_v", self.to_v)):
            m.weight.data.copy_(sd[n + ".weight"])
        self.to_out[0].weight.data.copy_(sd["to_out.0.weight"]); self.to_out[0].bias.data.copy_(sd["to_out.0.bias"])
        self.residual_connection, self.rescale_output_factor, self.spatial_norm, self.group_norm, self.norm_cross = False, 1.0, None, None, False


def test_attn_processor_seam_matches_reference_module_golden():
    """SURVEY 8b operator seam: HipAttnProcessor called with the reference processor's contract reproduces the outputs of the
    UNMODIFIED reference Attention module (golden), including injection through the returned handle and the averaged map."""
    import os
    from rich_text_to_image_amd.attention_processor import AttnMapHandle, HipAttnProcessor
    g = torch.load(os.path.join(os.path.dirname(__file__), "golden", "attention_ops.pt"))
    proc = HipAttnProcessor()
    x, x2, ctx = g["x"].to(DEV), g["x2"].to(DEV), g["ctx"].to(DEV)
    cross = _StubAttention(g["cross_sd"], 2, cross_dim=ctx.shape[-1])
    y, maps = proc(cross, x, encoder_hidden_states=ctx)
    report("processor cross plain", y, g["y_plain"], atol=3e-2, rtol=3e-2)
    assert maps[1].shape[-1] == 77 and maps[0].shape == (2, 256, 77)                       # what the hooks assert (rd.py:326,414)
    assert torch.allclose(maps[0].detach().cpu().sum(-1), torch.ones(2, 256), atol=2e-2)
    y, maps_fs = proc(cross, x, encoder_hidden_states=ctx, attn_weights={"word_pos": g["word_pos"], "font_size": g["font_size"]})
    report("processor cross font-size", y, g["y_fs"], atol=3e-2, rtol=3e-2)
    selfa = _StubAttention(g["self_sd"], 2)
    y, maps = proc(selfa, x)
    report("processor self", y, g["y_self"], atol=3e-2, rtol=3e-2)
    assert isinstance(maps[1], AttnMapHandle) and maps[1].shape == (4, 256, 256) and maps[1].detach() is maps[1]
    report("processor probs_avg", maps[0].detach().cpu(), g["p_self_avg"], atol=2e-3, rtol=5e-2)
    y, _ = proc(selfa, x2, real_attn_probs=maps[1])                                            # injection hook path (rd.py:366,382)
    report("processor self injected", y, g["y_inj"], atol=3e-2, rtol=3e-2)
    # a REAL probability tensor (what attention_processor.py:522-524 accepts): the reference module's own per-head probabilities of
    # `x`, recomputed in fp32 here, injected into the forward of `x2` must reproduce the same golden
    sd = g["self_sd"]
    q = F.linear(x.float().cpu(), sd["to_q.weight"]).reshape(2, 256, 2, -1).permute(0, 2, 1, 3).reshape(4, 256, -1)
    k = F.linear(x.float().cpu(), sd["to_k.weight"]).reshape(2, 256, 2, -1).permute(0, 2, 1, 3).reshape(4, 256, -1)
    probs = torch.softmax(q @ k.transpose(1, 2) * q.shape[-1] ** -0.5, -1).to(DEV)
    y, maps_r = proc(selfa, x2, real_attn_probs=probs)
    report("processor self injected (real probability tensor)", y, g["y_inj"], atol=3e-2, rtol=3e-2)
    assert maps_r[1] is probs
    report("processor probs_avg of a real tensor", maps_r[0].detach().cpu(), g["p_self_avg"], atol=2e-3, rtol=5e-2)
    with pytest.raises(TypeError):
        proc(selfa, x2, real_attn_probs=torch.zeros(4, 128, 256, device=DEV))


def test_attn_processor_probs_avg_on_a_token_grid_not_divisible_by_32():
    """20x20 = 400 tokens: the ragged self-attention kernel takes it (N % 8 == 0); the head-averaged map the token-map hooks read
    (rd.py:414-426) must too - the store kernel pads the key COUNT to 416, not the key rows."""
    from rich_text_to_image_amd.attention_processor import HipAttnProcessor
    C_, H, N = 64, 2, 400
    sd = {"to_q.weight": rnd(C_, C_, seed=1, scale=C_ ** -0.5), "to_k.weight": rnd(C_, C_, seed=2, scale=C_ ** -0.5),
          "to_v.weight": rnd(C_, C_, seed=3, scale=C_ ** -0.5), "to_out.0.weight": rnd(C_, C_, seed=4, scale=C_ ** -0.5), "to_out.0.bias": rnd(C_, seed=5)}
    x = rnd(1, N, C_, seed=6).to(DEV)
    y, maps = HipAttnProcessor()(_StubAttention(sd, H), x)
    q = F.linear(x.float().cpu(), sd["to_q.weight"]).reshape(1, N, H, -1).permute(0, 2, 1, 3)
    k = F.linear(x.float().cpu(), sd["to_k.weight"]).reshape(1, N, H, -1).permute(0, 2, 1, 3)
    ref = torch.softmax(q @ k.transpose(-1, -2) * q.shape[-1] ** -0.5, -1).mean(1)
    assert maps[0].shape == (1, N, N)
    report("probs_avg 400 tokens", maps[0].detach().cpu(), ref, atol=2e-3, rtol=5e-2)


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_attn_processor_inside_a_unet_forward(which):
    """The processor seam exercised the way the reference uses it (unet.set_attn_processor + the hook families of
    region_diffusion*.py): EVERY attention module of a UNet forward goes through HipAttnProcessor - cross-attention with the
    font-size dict, self-attention whose returned handle is captured on a `text_ref` forward and passed back as real_attn_probs on
    a region forward - while everything else stays the fp32 oracle.  Reference: the same forwards with the oracle's own attention."""
    import sys, os
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
    from oracle.unet import OracleUNet, TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict
    from rich_text_to_image_amd.attention_processor import HipAttnProcessor
    xl = which == "xl"
    cfg = TINY_XL_CONFIG if xl else TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=11)
    hw = 32
    g = torch.Generator().manual_seed(77)
    D = cfg["cross_attention_dim"]
    emb = torch.randn(2, 77, D, generator=g)
    pooled = torch.randn(2, 32, generator=g) if xl else None
    tid = torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]]) if xl else None
    lat, lat_ref = torch.randn(1, 4, hw, hw, generator=g), torch.randn(1, 4, hw, hw, generator=g)
    fsd = {"word_pos": torch.tensor([2, 6]), "font_size": torch.tensor([3.0, -1.5])}

    def added(k):
        return {"text_embeds": pooled[k:k + 1], "time_ids": tid} if xl else None

    def run(o):
        with torch.no_grad():
            a = o.forward(lat, 500.0, emb[:1], added(0), ctl={"fontsize": fsd})
            cap = {}
            b = o.forward(lat_ref, 500.0, emb[1:2], added(1), ctl={"capture": cap})
            inj = {k: v for k, v in cap.items() if k.endswith("attn1")}
            c = o.forward(lat, 500.0, emb[1:2], added(1), ctl={"inject": inj})
        return a, b, c
    ref = run(OracleUNet(cfg, sd))

    proc, mods, calls = HipAttnProcessor(), {}, {"self": 0, "cross": 0, "injected": 0}

    def impl(o, name, x, heads, ctx, fontsize, real_probs):
        if name not in mods:
            lsd = {k[len(name) + 1:]: v for k, v in o.sd.items() if k.startswith(name + ".")}
            mods[name] = _StubAttention(lsd, heads, cross_dim=None if ctx is None else ctx.shape[-1])
        y, maps = proc(mods[name], x.to(DEV), real_attn_probs=real_probs, attn_weights=fontsize,
                       encoder_hidden_states=None if ctx is None else ctx.to(DEV))
        calls["cross" if ctx is not None else ("injected" if real_probs is not None else "self")] += 1
        return y.float().cpu(), maps[1]                      # what the hooks keep: out[1][1] (rd.py:366,382 / xl.py:1064-1106)
    o2 = OracleUNet(cfg, sd)
    o2.attn_impl = impl
    got = run(o2)
    assert calls["self"] > 0 and calls["cross"] > 0 and calls["injected"] > 0 and calls["injected"] * 2 == calls["self"]
    for name, a, b in zip(("font-size", "text_ref (captured)", "region (injected)"), got, ref):
        r = ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()
        print(f"{which} processor inside the UNet, {name}: rel-L2 {r:.3e}")
        assert r < 1.5e-2, name


def test_attn_processor_probs_avg_at_4096_tokens():
    """SDXL's first attention level has 64x64 = 4096 tokens and the XL token-map hook reads probs_avg of EVERY attn1 layer
    (region_diffusion_sdxl.py:980-992): the averaged map must exist there too (keys are processed in 1024-key chunks)."""
    from rich_text_to_image_amd.attention_processor import HipAttnProcessor
    H, d, N, Cc = 2, 64, 4096, 128
    g = torch.Generator().manual_seed(5)
    sd = {"to_q.weight": torch.randn(H * d, Cc, generator=g) * Cc ** -0.5 * 2, "to_k.weight": torch.randn(H * d, Cc, generator=g) * Cc ** -0.5 * 2,
          "to_v.weight": torch.randn(H * d, Cc, generator=g) * Cc ** -0.5, "to_out.0.weight": torch.randn(Cc, H * d, generator=g) * (H * d) ** -0.5,
          "to_out.0.bias": torch.zeros(Cc)}
    x = torch.randn(1, N, Cc, generator=g)
    proc = HipAttnProcessor()
    y, maps = proc(_StubAttention(sd, H), x.to(DEV))
    assert maps[0] is not None and maps[0].shape == (1, N, N)
    got = maps[0].detach().cpu()
    xb = x.to(torch.bfloat16).float()
    q = F.linear(xb, sd["to_q.weight"].to(torch.bfloat16).float()).reshape(1, N, H, d).permute(0, 2, 1, 3)
    k = F.linear(xb, sd["to_k.weight"].to(torch.bfloat16).float()).reshape(1, N, H, d).permute(0, 2, 1, 3)
    ref = torch.softmax(q @ k.transpose(-1, -2) * d ** -0.5, -1).mean(1)
    assert torch.allclose(got.sum(-1), torch.ones(1, N), atol=2e-2)
    rel = ((got - ref).pow(2).sum() / ref.pow(2).sum()).sqrt().item()
    print(f"probs_avg 4096x4096: rel-L2 {rel:.3e}")
    assert rel < 3e-2
