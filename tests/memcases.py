"""The GEMM / convolution case table of the memory-contract tests, shared by tests/test_gemm_route.py (CPU: every case takes the route it
is listed under, asked through rt_op_gemm_route) and tests/test_memory_contract_gpu.py (GPU: runs them); further down HILO_CASES, the
VAE's hi / lo contraction behind rt_op_gemm_hilo (route query: rt_op_gemm_hilo_route; GPU: tests/test_vae_ops_gpu.py).  Plain data, no torch.

A case is one rt_op_gemm call: `mode` 0 dense [M, N, K] | 1 / 2 / 3 a 3x3 convolution (stride 1 / stride 2 / nearest-2x up-sample folded
in) of a [B, H, W, Cin] image to Cout channels; `epi` as rt_op_gemm; `cfg` = rt_op_gemm_force_config, `debug` = rt_op_gemm_debug word
while it runs; `bias` False: no bias.  `kind` is the route it must take, `var` (optional) the tile variant / configuration and `slices`
(optional) the slice count.

rt_op_gemm passes no stream shares (split_tiles = 0), so the split rule counts the ACTUAL 128 x 128 tiles of the problem: anything with
<= 96 tiles and K >= 512 is sliced.  The convolution cases that must NOT be sliced (PATCH, G16) are therefore sized to > 96 tiles - or,
for the implicit GEMM on a tile configuration, to K < 512 (Cin = 48 / 8) - and the small 64-channel shapes appear under KSPLIT instead.
"""
TILE, G16, G16_UP2, PATCH, PATCH_SPLIT, KSPLIT, TRIPLE = range(7)
KIND_NAMES = ["TILE", "G16", "G16_UP2", "PATCH", "PATCH_SPLIT", "KSPLIT", "TRIPLE"]
NO_CHUNK_SPLIT = 1 << 28          # rt_op_gemm_debug bit 28: under-filled 3x3 convolutions on the split-K implicit GEMM
GEGLU_CFGS = (0, 1, 3, 5, 7)      # tile configurations with a GEGLU epilogue (kCfg[].geglu_ok); a forced other one falls back to 0

# (route kind, epilogue) pairs that exist behind rt_op_gemm / rt_op_upconv - from launch_routed / launch_with_cfg / launch_conv3p /
# splitk_reduce_kernel / gemm16_supported.  TRIPLE (the precise VAE's hi / lo contraction) needs GemmArgs.A_lo, which rt_op_gemm does not
# take: it and the one-launch hi / lo forms are reached through rt_op_gemm_hilo (HILO_CASES / HILO_FORMS below).  G16_UP2 needs the phase
# pack, which only rt_op_upconv passes (it reports the route itself as *phase_route; UPCONV_CASES below).
IMPLEMENTED = {
    TILE: {0, 1, 2, 3, 4},
    G16: {0, 1, 2, 3, 4},          # 2: the convolution form (time embedding); 3: dense GEGLU
    G16_UP2: {4},
    PATCH: {0, 1, 2, 4},
    PATCH_SPLIT: {0, 1, 2, 4},     # the reduction's epilogues a convolution can ask for
    KSPLIT: {0, 1, 2, 3, 4},
}


def dense(kind, epi, M, N, K, cfg=-1, debug=0, bias=True, rpb=0, **kw):
    return dict(kind=kind, mode=0, epi=epi, M=M, N=N, K=K, cfg=cfg, debug=debug, bias=bias, rpb=rpb, **kw)


def conv(kind, mode, epi, B, H, W, Cin, Cout, cfg=-1, debug=0, **kw):
    return dict(kind=kind, mode=mode, epi=epi, B=B, H=H, W=W, Cin=Cin, Cout=Cout, cfg=cfg, debug=debug, bias=True, **kw)


def conv_out_hw(c):
    if c["mode"] == 1:
        return c["H"], c["W"]
    if c["mode"] == 2:
        return (c["H"] + 1) // 2, (c["W"] + 1) // 2
    return 2 * c["H"], 2 * c["W"]


def case_id(c):
    tail = (f"-cfg{c['cfg']}" if c["cfg"] >= 0 else "") + (f"-dbg{c['debug']:x}" if c["debug"] else "") + ("" if c["bias"] else "-nobias")
    if c["mode"] == 0:
        return f"{KIND_NAMES[c['kind']]}-dense-{c['M']}x{c['N']}x{c['K']}-epi{c['epi']}{tail}"
    return f"{KIND_NAMES[c['kind']]}-conv{c['mode']}-{c['B']}x{c['H']}x{c['W']}x{c['Cin']}to{c['Cout']}-epi{c['epi']}{tail}"


def route_args(c, pad=0):
    """(mode, epi, M, N, K, lda, ldw, ldo, rows_per_batch, Hin, Win, Cin, Hout, Wout) of the case; pad > 0: the contract run's leading dimensions."""
    if c["mode"] == 0:
        oc = c["N"] // 2 if c["epi"] == 3 else c["N"]
        return (0, c["epi"], c["M"], c["N"], c["K"], c["K"] + pad, c["K"] + pad, oc + pad, c["rpb"], 0, 0, 0, 0, 0)
    Ho, Wo = conv_out_hw(c)
    K = 9 * c["Cin"]
    return (c["mode"], c["epi"], c["B"] * Ho * Wo, c["Cout"], K, 0, K + pad, c["Cout"] + pad, Ho * Wo, c["H"], c["W"], c["Cin"], Ho, Wo)


GEMM_CASES = []
# ---- dense on a gemm.hip tile configuration, each forced configuration 0..8: ragged in M (300 = 2 x 128 + 44 = 256 + 44), N (200) and K
#      (200 = 3 x 64 + 8: the K tail goes through the zero page); GEGLU at N = 192 for the configurations that have it
for _cfg in range(9):
    GEMM_CASES += [dense(TILE, 0, 300, 200, 200, cfg=_cfg, var=_cfg), dense(TILE, 1, 300, 200, 200, cfg=_cfg, var=_cfg),
                   dense(TILE, 2, 300, 200, 200, cfg=_cfg, var=_cfg, rpb=100), dense(TILE, 4, 300, 200, 200, cfg=_cfg, var=_cfg)]
    if _cfg in GEGLU_CFGS:
        GEMM_CASES.append(dense(TILE, 3, 300, 192, 200, cfg=_cfg, var=_cfg))
GEMM_CASES.append(dense(TILE, 1, 300, 200, 200, var=0))                    # ... and what the shape rule itself picks
# ---- dense split-K: every epilogue of splitk_reduce_kernel (2 slices by the actual tile count: 1 x 4 tiles), and one without bias
GEMM_CASES += [dense(KSPLIT, e, 72, 512, 512, slices=2, rpb=24 if e == 2 else 0) for e in range(5)]
GEMM_CASES += [dense(KSPLIT, 3, 72, 512, 512, slices=2, bias=False), dense(KSPLIT, 4, 72, 512, 512, slices=2, bias=False)]
# ---- dense through the shape rule onto gemm16.hip (the variants themselves: G16_VARIANT_CASES): class A 128 x 256, class B 64 x 160, GEGLU
GEMM_CASES += [dense(G16, 0, 300, 256, 256, var=8), dense(G16, 1, 300, 320, 256, var=9), dense(G16, 4, 300, 320, 256, var=9),
               dense(G16, 3, 300, 512, 256)]
# ---- 3x3 convolutions on the patch kernel (112 tiles: not sliced), ragged last column tile (136 = 96 + 40)
GEMM_CASES += [conv(PATCH, 1, e, 1, 64, 112, 64, 136) for e in (0, 1, 2, 4)]
GEMM_CASES += [conv(PATCH, 3, e, 1, 32, 56, 64, 136) for e in (1, 4)]
# ---- implicit GEMM on a tile configuration: sides that are no multiple of 16, K < 512; Cin = 8 (one 8-channel chunk per tap); stride 2
#      with odd input sides (odd 6 x 10 output)
GEMM_CASES += [conv(TILE, 1, 1, 1, 8, 24, 48, 72), conv(TILE, 1, 4, 1, 8, 24, 48, 72), conv(TILE, 1, 0, 1, 8, 24, 8, 72),
               conv(TILE, 1, 2, 1, 8, 24, 8, 72), conv(TILE, 2, 1, 2, 11, 19, 48, 64), conv(TILE, 2, 4, 2, 12, 20, 48, 64),
               conv(TILE, 3, 1, 1, 8, 8, 48, 96), conv(TILE, 3, 4, 1, 8, 8, 48, 96)]
# ---- implicit GEMM on gemm16.hip's main loop (one image: 8 x 4 tiles of 224 x 160 >= 30; two images: 130 tiles, not sliced), sides 36 x 46
GEMM_CASES += [conv(G16, 1, e, 2, 36, 46, 128, 640, var=0) for e in (0, 1, 2, 4)]
# ---- the patch kernel split over its input-channel chunks + reduction: the small one for every epilogue, SD-v1.5's 16 x 16 level, the
#      two-halves form one level up (120 tiles: not sliced by the K rule), and the up-sample form
GEMM_CASES += [conv(PATCH_SPLIT, 1, e, 1, 16, 16, 512, 64, slices=8) for e in (0, 1, 2, 4)]
GEMM_CASES += [conv(PATCH_SPLIT, 1, 4, 3, 16, 16, 1280, 1280, slices=7), conv(PATCH_SPLIT, 1, 4, 3, 32, 32, 512, 640, slices=2),
               conv(PATCH_SPLIT, 3, 4, 1, 8, 8, 512, 64, slices=8)]
# ---- the same problems on the split-K implicit GEMM (debug bit 28), and the small shapes the K rule slices by itself
GEMM_CASES += [conv(KSPLIT, 1, 4, 3, 16, 16, 1280, 1280, debug=NO_CHUNK_SPLIT), conv(KSPLIT, 1, 2, 1, 16, 16, 512, 64, debug=NO_CHUNK_SPLIT),
               conv(KSPLIT, 1, 0, 1, 16, 32, 64, 96), conv(KSPLIT, 1, 1, 1, 8, 24, 64, 72), conv(KSPLIT, 2, 1, 2, 12, 20, 64, 64),
               conv(KSPLIT, 3, 4, 1, 8, 8, 64, 96), conv(KSPLIT, 1, 4, 3, 20, 24, 128, 160), conv(KSPLIT, 1, 2, 3, 20, 24, 128, 160)]

# ---------------------------------------------------------------------------------------------------------------------------------------
# rt_op_gemm_hilo: the VAE's contraction A W + A_lo W + A W_lo (fp32 output, ONE image, prefer_patch_conv by the VAE's own rule).  `kind`
# is what rt_op_gemm_hilo_route reports for the hi / lo call - the route of the ONE launch that runs the three passes (G16 dense, PATCH
# convolutions), or TRIPLE - and `pass_kind` the route of each of TRIPLE's three launches (= kind for the fused forms).  mode 0 dense |
# 1 stride-1 conv | 3 up-2 conv | 4 stride-2 conv with bottom / right padding.  res: None | "res" | "inplace" (out == res, attn_bwd's
# accumulation); pair: the bf16 pair output (patch kernel only); wact: W is an activation pair (attention products: no bias).
# Where a candidate shape of the issue landed elsewhere it is listed where it landed (see the notes next to it).
TRIPLE_ALL, TRIPLE_PATCH, TRIPLE_DENSE = 1 << 7, 1 << 9, 1 << 15          # rt_op_gemm_debug bits 7 / 9 / 15: the fused forms as three launches


def hdense(kind, pass_kind, M, N, K, debug=0, bias=True, res=None, wact=False):
    return dict(kind=kind, pass_kind=pass_kind, mode=0, M=M, N=N, K=K, debug=debug, bias=bias and not wact, res=res, pair=False, wact=wact)


def hconv(kind, pass_kind, mode, H, W, Cin, Cout, debug=0, bias=True, res=None, pair=False):
    return dict(kind=kind, pass_kind=pass_kind, mode=mode, H=H, W=W, Cin=Cin, Cout=Cout, debug=debug, bias=bias, res=res, pair=pair, wact=False)


def hilo_out_hw(c):
    return {1: (c["H"], c["W"]), 3: (2 * c["H"], 2 * c["W"]), 4: (c["H"] // 2, c["W"] // 2)}[c["mode"]]


def hilo_id(c):
    tail = (f"-dbg{c['debug']:x}" if c["debug"] else "") + ("" if c["bias"] else "-nobias") + (f"-{c['res']}" if c["res"] else "") + ("-pair" if c["pair"] else "")
    head = KIND_NAMES[c["kind"]] + ("" if c["pass_kind"] == c["kind"] else "/" + KIND_NAMES[c["pass_kind"]])
    if c["mode"] == 0:
        return f"{head}-dense-{c['M']}x{c['N']}x{c['K']}{tail}"
    return f"{head}-conv{c['mode']}-{c['H']}x{c['W']}x{c['Cin']}to{c['Cout']}{tail}"


def hilo_route_args(c, pad=0, hilo=True):
    """(hilo, pair, mode, M, N, K, lda, ldw, ldo, rows_per_batch, Hin, Win, Cin, Hout, Wout) of rt_op_gemm_hilo_route."""
    if c["mode"] == 0:
        return (int(hilo), 0, 0, c["M"], c["N"], c["K"], c["K"] + pad, c["K"] + pad, c["N"] + pad, 0, 0, 0, 0, 0, 0)
    Ho, Wo = hilo_out_hw(c)
    K = 9 * c["Cin"]
    return (int(hilo), int(c["pair"]), c["mode"], Ho * Wo, c["Cout"], K, 0, K + pad, c["Cout"] + pad, Ho * Wo, c["H"], c["W"], c["Cin"], Ho, Wo)


HILO_CASES = []
# ---- fused dense on the 16x16x32 family, with a residual, accumulating in place, and without bias
HILO_CASES += [hdense(G16, G16, 300, 256, 256), hdense(G16, G16, 300, 256, 256, res="res"), hdense(G16, G16, 300, 256, 256, res="inplace", bias=False)]
# ---- three launches of a gemm.hip tile configuration: K tail through the zero page in both planes (200 = 3 x 64 + 8); the attention
#      products with activation pairs on both sides; Cin = 8; the encoder's stride-2 convolution (Cin = 48: K = 432 < 512 is not sliced - the
#      issue's 1 x 12 x 20 x 64 -> 64 has K = 576 and 1 tile: two K slices, listed under KSPLIT below)
HILO_CASES += [hdense(TRIPLE, TILE, 300, 200, 200), hdense(TRIPLE, TILE, 300, 200, 200, res="inplace", bias=False),
               hdense(TRIPLE, TILE, 240, 240, 64, wact=True), hdense(TRIPLE, TILE, 240, 64, 240, wact=True),
               hconv(TRIPLE, TILE, 1, 8, 24, 8, 72), hconv(TRIPLE, TILE, 4, 12, 20, 48, 64)]
# ---- three launches of the split-K form (the K rule slices each pass): dense, a small 64-channel convolution, conv_out's N = 4
HILO_CASES += [hdense(TRIPLE, KSPLIT, 72, 512, 512), hdense(TRIPLE, KSPLIT, 72, 512, 512, res="res"),
               hconv(TRIPLE, KSPLIT, 1, 16, 16, 64, 96), hconv(TRIPLE, KSPLIT, 1, 16, 16, 64, 4), hconv(TRIPLE, KSPLIT, 4, 12, 20, 64, 64)]
# ---- the patch kernel's one-launch form: with / without residual, with / without the pair output; behind the 2x up-sample
HILO_CASES += [hconv(PATCH, PATCH, 1, 64, 112, 64, 136), hconv(PATCH, PATCH, 1, 64, 112, 64, 136, res="res"),
               hconv(PATCH, PATCH, 1, 64, 112, 64, 136, pair=True), hconv(PATCH, PATCH, 1, 64, 112, 64, 136, bias=False, pair=True),
               hconv(PATCH, PATCH, 3, 32, 56, 64, 136), hconv(PATCH, PATCH, 3, 32, 56, 64, 136, res="res")]
# ---- every fused form again as three launches (debug bits 7, 9, 15); the pair output survives on the patch kernel's single passes
HILO_CASES += [hdense(TRIPLE, G16, 300, 256, 256, debug=TRIPLE_DENSE), hdense(TRIPLE, G16, 300, 256, 256, debug=TRIPLE_ALL, res="res"),
               hdense(TRIPLE, G16, 300, 256, 256, debug=TRIPLE_DENSE, res="inplace", bias=False),
               hconv(TRIPLE, PATCH, 1, 64, 112, 64, 136, debug=TRIPLE_PATCH, res="res"), hconv(TRIPLE, PATCH, 1, 64, 112, 64, 136, debug=TRIPLE_ALL),
               hconv(TRIPLE, PATCH, 3, 32, 56, 64, 136, debug=TRIPLE_PATCH), hconv(TRIPLE, PATCH, 3, 32, 56, 64, 136, debug=TRIPLE_ALL, res="res")]
# the forms of the hi / lo contraction that exist: each needs a case (tests/test_gemm_route.py)
HILO_FORMS = {(G16, G16), (PATCH, PATCH), (TRIPLE, TILE), (TRIPLE, KSPLIT), (TRIPLE, G16), (TRIPLE, PATCH)}

# rt_op_gemm16_variant (no routing: the caller names the tile): (variant, N, weights_on_rows, epilogues), M = 300 / K = 256 everywhere.
# One class A variant per tile height (3: 256 rows, 2: 224, 8: 128, 11: 64), the class B variants 0, 1, 9, the V^T variants 6, 7, 12.
G16_M, G16_K = 300, 256
G16_VARIANT_CASES = [(3, 256, 0, (0, 1, 3, 4)), (2, 256, 0, (0, 1, 3, 4)), (8, 256, 0, (0, 1, 3, 4)), (11, 320, 0, (0, 1, 4)),
                     (0, 160, 0, (0, 1, 4)), (1, 160, 0, (0, 1, 4)), (9, 160, 0, (0, 1, 4)),
                     (6, 296, 1, (0,)), (7, 296, 1, (0,)), (12, 296, 1, (0,))]     # V^T: M = 320 weight rows (M % 160 == 0), N = 296 tokens

# rt_op_upconv: (B, H, W, Cin, Cout, with_phase_pack, expected *phase_route): 40 x 48 low-resolution pixels = 9 row tiles x 4 column
# tiles of 224 x 160 >= 30 -> the four-phase launch; without the pack the patch kernel (H, W multiples of 8: 16 x 16 output patches)
UPCONV_CASES = [(1, 40, 48, 64, 640, True, 1), (1, 40, 48, 64, 640, False, 0)]
