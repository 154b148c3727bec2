"""Upsample2D's convolution as four 2x2 phase convolutions of the low-resolution map (csrc/gemm16.hip, MODE = A_CONV3_UP2; include/rtdiff.h:
rt_op_pack_upconv / rt_op_upconv / rt_op_gemm_debug2).

conv3x3(nearest-2x(x)) at output pixel (2y + a, 2x + b) reads only the input pixels (y + a - 1 + r, x + b - 1 + c), r, c in {0, 1}; the phase
weights are sums of the 3x3 taps, formed in fp32 from the SOURCE tensor and rounded to bf16 once.

Kernel level: both routes against F.conv2d(F.interpolate(x)) with the UNROUNDED fp32 weights on bf16-exact activations, the whole output
(borders included).  What separates either route from that reference is the bf16 rounding of its weights (9 taps rounded one by one, or 4 sums
rounded once: 0.94 - 1.03 x the same rel-L2 in fp64 on the CPU), the fp32 accumulation order and the fp16 rounding of the output, the last two common
to both.  Condition: rel-L2(phase route) <= 1.1 x rel-L2(patch-kernel route); the 1.1 covers sampling spread only.

Shapes: SDXL's two up-samplers with the 7 streams of a rich-text step and with one stream alone, and a non-square map.  The tile rule of the
phase route (gemm16_pick_up2) asks ONE image's low-resolution map for >= 30 tiles of 224 x 160 (or >= 32 of 224 x 320), like the 3x3
convolutions of the same family: 16 x 24 at 320 channels gives 4 and stays on the patch kernel; 40 x 48 at 640 channels (9 x 4 = 36 tiles, the
last row tile partial: 1920 = 8 x 224 + 128 rows) takes the phase route.

Engine level: one full-architecture SDXL forward on each route against the committed fp32 oracle output of tests/test_fullsize_gpu.py
(distance = root mean square of the four streams' rel-L2), condition new <= 1.05 x old; and a second engine that received only a byte copy of the
first engine's arena + rt_arena_mark_bound must give the same bits (the phase pack lives in the arena that a multi-GPU launch broadcasts).
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hiputil import DEV, bf, chk, gemm  # noqa: E402
from upconv_ref import phase_pack_ref  # noqa: E402


def _lib():
    from rich_text_to_image_amd.engine import load_library
    return load_library()


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


def pack9(w):
    """[Cout, Cin, 3, 3] -> bf16 [Cout, 9 Cin], K index = tap * Cin + c (the engine's 3x3 pack)."""
    return bf(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1))


def pack_phase(w):
    lib = _lib()
    Cout, Cin = w.shape[:2]
    wd = w.to(DEV).contiguous()
    out = torch.empty(4, Cout, 4 * Cin, device=DEV, dtype=torch.bfloat16)
    chk(lib.rt_op_pack_upconv(_ptr(wd), 0, Cout, Cin, _ptr(out), None))
    torch.cuda.synchronize()
    return out


def upconv(x_nhwc, w9, wph, bias, N):
    """-> (fp16 [B, 2H, 2W, N], 1 if the four-phase launch ran)."""
    lib = _lib()
    B, H, W_, Cin = x_nhwc.shape
    out = torch.empty(B, 2 * H, 2 * W_, N, device=DEV, dtype=torch.float16)
    route = C.c_int(-1)
    chk(lib.rt_op_upconv(_ptr(x_nhwc), _ptr(w9), _ptr(wph), _ptr(bias), _ptr(out), B, H, W_, Cin, N, C.byref(route), None))
    torch.cuda.synchronize()
    return out, route.value


def _problem(B, H, W_, Cin, Cout, seed):
    x = rnd(B, Cin, H, W_, seed=seed).to(torch.bfloat16)                         # bf16-exact activations
    w = rnd(Cout, Cin, 3, 3, seed=seed + 1, scale=(9 * Cin) ** -0.5)            # fp32, NOT rounded
    bias = rnd(Cout, seed=seed + 2).to(DEV)
    return x, w, bias


def _reference(x, w, bias):
    tf32 = torch.backends.cudnn.allow_tf32
    torch.backends.cudnn.allow_tf32 = False
    try:
        ref = F.conv2d(F.interpolate(x.float().to(DEV), scale_factor=2.0, mode="nearest"), w.to(DEV), bias, padding=1)
    finally:
        torch.backends.cudnn.allow_tf32 = tf32
    return ref.permute(0, 2, 3, 1).contiguous()


def test_phase_pack_matches_fp32_restatement():
    """rt_op_pack_upconv = the fp32 sums of the source taps (ky-major, kx-minor), rounded once: bit for bit, fp32 / fp16 / bf16 sources."""
    lib = _lib()
    w = rnd(96, 64, 3, 3, seed=5, scale=0.05)
    for dt, code in ((torch.float32, 0), (torch.float16, 1), (torch.bfloat16, 2)):
        wd = w.to(dt).to(DEV).contiguous()
        out = torch.empty(4, 96, 4 * 64, device=DEV, dtype=torch.bfloat16)
        chk(lib.rt_op_pack_upconv(_ptr(wd), code, 96, 64, _ptr(out), None))
        torch.cuda.synchronize()
        ref = phase_pack_ref(w.to(dt).float()).to(torch.bfloat16)
        assert torch.equal(out.cpu(), ref), dt


SHAPES = [(7, 32, 32, 1280, 1280), (7, 64, 64, 640, 640), (1, 32, 32, 1280, 1280), (1, 64, 64, 640, 640), (2, 40, 48, 640, 640)]


@pytest.mark.parametrize("B,H,W_,Cin,Cout", SHAPES)
def test_phase_route_is_as_accurate_as_the_patch_route(B, H, W_, Cin, Cout):
    x, w, bias = _problem(B, H, W_, Cin, Cout, seed=31)
    A, w9, wph = bf(x.permute(0, 2, 3, 1)), pack9(w), pack_phase(w)
    ref = _reference(x, w, bias)
    new, r_new = upconv(A, w9, wph, bias, Cout)
    old, r_old = upconv(A, w9, None, bias, Cout)                                  # no phase pack: today's patch kernel (rt_op_gemm mode 3)
    assert r_new == 1 and r_old == 0
    e_new, e_old = rel_l2(new, ref), rel_l2(old, ref)
    print(f"upconv {B}x{H}x{W_}x{Cin}->{Cout}: rel-L2 vs fp32 weights: phase route {e_new:.4e}, patch route {e_old:.4e}, ratio {e_new / e_old:.3f}; "
          f"phase vs patch {rel_l2(new, old):.4e}")
    assert torch.isfinite(new.float()).all()
    assert e_new <= 1.1 * e_old, (e_new, e_old)
    # the borders on their own (first / last two output rows and columns: every padding tap)
    edge = torch.zeros(2 * H, 2 * W_, dtype=torch.bool, device=DEV)
    edge[:2] = edge[-2:] = True
    edge[:, :2] = edge[:, -2:] = True
    b_new, b_old = rel_l2(new[:, edge], ref[:, edge]), rel_l2(old[:, edge], ref[:, edge])
    print(f"  borders: phase route {b_new:.4e}, patch route {b_old:.4e}")
    assert b_new <= 1.1 * b_old, (b_new, b_old)


@pytest.mark.parametrize("B,H,W_,Cin,Cout", [(7, 32, 32, 1280, 1280), (7, 64, 64, 640, 640)])
def test_phase_route_is_deterministic_and_batch_invariant(B, H, W_, Cin, Cout):
    x, w, bias = _problem(B, H, W_, Cin, Cout, seed=41)
    A, w9, wph = bf(x.permute(0, 2, 3, 1)), pack9(w), pack_phase(w)
    o1, r1 = upconv(A, w9, wph, bias, Cout)
    o2, r2 = upconv(A, w9, wph, bias, Cout)
    assert r1 == 1 and r2 == 1
    assert torch.equal(o1, o2)
    for b in (0, 3, B - 1):                                                       # a stream alone = the same stream inside the batch of 7
        ob, rb = upconv(A[b:b + 1].contiguous(), w9, wph, bias, Cout)
        assert rb == 1
        assert torch.equal(ob[0], o1[b]), b


def test_shapes_outside_the_family_keep_the_patch_route_bit_for_bit():
    lib = _lib()
    for (B, H, W_, Cin, Cout) in [(2, 16, 16, 64, 96), (1, 16, 24, 320, 320)]:
        x, w, bias = _problem(B, H, W_, Cin, Cout, seed=51)
        A, w9, wph = bf(x.permute(0, 2, 3, 1)), pack9(w), pack_phase(w)
        before = gemm(A, w9, bias, epi=4, mode=3, conv=(2 * H, 2 * W_)).reshape(B, 2 * H, 2 * W_, Cout)     # the unchanged entry: no phase pack in sight
        on, r_on = upconv(A, w9, wph, bias, Cout)
        try:
            chk(lib.rt_op_gemm_debug2(1))
            off, r_off = upconv(A, w9, wph, bias, Cout)
        finally:
            chk(lib.rt_op_gemm_debug2(0))
        assert r_on == 0 and r_off == 0
        assert torch.equal(on, before) and torch.equal(off, before)


def test_switch_restores_the_patch_route():
    lib = _lib()
    B, H, W_, Cin, Cout = 1, 32, 32, 1280, 1280
    x, w, bias = _problem(B, H, W_, Cin, Cout, seed=61)
    A, w9, wph = bf(x.permute(0, 2, 3, 1)), pack9(w), pack_phase(w)
    before = gemm(A, w9, bias, epi=4, mode=3, conv=(2 * H, 2 * W_)).reshape(B, 2 * H, 2 * W_, Cout)
    try:
        chk(lib.rt_op_gemm_debug2(1))
        off, r_off = upconv(A, w9, wph, bias, Cout)
    finally:
        chk(lib.rt_op_gemm_debug2(0))
    assert r_off == 0 and torch.equal(off, before)


# ----------------------------------------------------------------------------------------------- engine level
@pytest.fixture(scope="module")
def sdxl():
    from oracle.unet import SDXL_CONFIG
    from test_fullsize_gpu import _build
    eng, o = _build(SDXL_CONFIG, 128, 128, 21, max_streams=8, max_prompts=8)
    yield eng, o
    eng.close()


def test_sdxl_forward_distance_from_the_oracle_on_both_routes(sdxl):
    """Recorded on MI355X (rms over the four streams of rel-L2 against the fp32 oracle): see the printed line; condition new <= 1.05 x old."""
    from oracle.unet import SDXL_CONFIG
    from test_fullsize_gpu import _stream_mode_forward
    lib = _lib()
    eng, o = sdxl

    def dist(res):
        return (sum(v * v for v in res.values()) / len(res)) ** 0.5
    new = _stream_mode_forward(eng, o, SDXL_CONFIG, 128, 128, True, 801.0)
    try:
        chk(lib.rt_op_gemm_debug2(1))
        old = _stream_mode_forward(eng, o, SDXL_CONFIG, 128, 128, True, 801.0)
    finally:
        chk(lib.rt_op_gemm_debug2(0))
    print(f"SDXL forward vs fp32 oracle: phase route {dist(new):.4e} {new}, patch route {dist(old):.4e} {old}, ratio {dist(new) / dist(old):.4f}")
    assert new != old                                                             # the switch really changes the route
    assert dist(new) <= 1.05 * dist(old), (new, old)


def test_engine_fed_by_an_arena_copy_gives_the_same_bits(sdxl):
    from oracle.unet import SDXL_CONFIG
    from rich_text_to_image_amd.engine import Engine
    from rich_text_to_image_amd.launcher import arena_tensor
    eng, _ = sdxl
    g = torch.Generator().manual_seed(7)
    emb, pooled = torch.randn(2, 77, SDXL_CONFIG["cross_attention_dim"], generator=g), torch.randn(2, 1280, generator=g)
    tid = torch.tensor([[1024.0, 1024.0, 0, 0, 1024.0, 1024.0]])
    x = torch.randn(2, 4, 128, 128, generator=g).to(DEV)
    dst = Engine(SDXL_CONFIG, 128, 128, device=0, max_streams=8, max_prompts=8)
    try:
        assert dst.weights_missing()[0] > 0
        a, b = arena_tensor(eng), arena_tensor(dst)
        assert a.numel() == b.numel()
        b.copy_(a)
        torch.cuda.synchronize()
        dst.arena_mark_bound()
        outs = []
        for e in (eng, dst):
            e.set_prompts(emb.to(DEV), pooled.to(DEV), tid)
            e.set_fontsize(None, None)
            outs.append(e.unet_forward(x, 500.0, [0, 1]).clone())
        assert torch.isfinite(outs[0]).all()
        assert torch.equal(outs[0], outs[1])
    finally:
        dst.close()
