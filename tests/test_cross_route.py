"""The route of an attn2 launch (csrc/engine.hip::cross_route through rt_op_cross_route; no GPU): which kernel runs a cross-attention launch
of the UNet forward and whether it may hand its softmax statistics to the token-map store.  The forward and every operator entry that
launches cross-attention decide through that one function, so the table below pins them all.  A route is a function of the layer's
shape and of the streams' key counts, never of the cache's capacity (prompt_rows is only the stride between prompts)."""
import ctypes as C

import pytest

from hiputil import cross_route

GENERIC, CROSS77, RUNS, XATTN_FUSED, XBLOCK = range(5)
ATTN, C77, CMW = 0, 1, 2                                  # kernel of a stream
B4, B16, B17, B19 = 1 << 4, 1 << 16, 1 << 17, 1 << 19     # rt_op_gemm_debug: no fused to_q launch / xblock / store's own statistics / no cross77_kernel

L640 = dict(C_=640, heads=10, d=64, DP=64, tokens=4096)       # SDXL's 640-channel level at 64 x 64
L1280 = dict(C_=1280, heads=20, d=64, DP=64, tokens=1024)     # ... its 1280-channel level at 32 x 32
SD15 = dict(C_=320, heads=8, d=40, DP=64, tokens=4096)        # SD-v1.5: heads of 40, padded to 64
# name -> (layer, prompt rows, key counts, kind, kernel of every stream)
ROWS = {
    "a: 640 ch, 7 x 77 keys": (L640, 96, [77] * 7, CROSS77, [C77] * 7),
    "c: 1280 ch, mixed counts": (L1280, 192, [77, 154, 77, 77], RUNS, [C77, CMW, C77, C77]),
    "d: 1280 ch, all 77 in a 192-row cache": (L1280, 192, [77] * 4, CROSS77, [C77] * 4),
    "e: 1280 ch, 2 x 231 keys": (L1280, 288, [231, 231], RUNS, [CMW, CMW]),
    "f: 1280 ch, 3 x 154 keys": (L1280, 192, [154] * 3, RUNS, [CMW] * 3),
    "g: d = 40 padded to 64": (SD15, 96, [77] * 3, GENERIC, [ATTN] * 3),
    "h: that shape with d given as DP (an entry without d)": (dict(SD15, d=64), 96, [77] * 3, CROSS77, [C77] * 3),
    "i: d = 80 / DP = 96": (dict(C_=640, heads=8, d=80, DP=96, tokens=1024), 96, [77] * 3, GENERIC, [ATTN] * 3),
    "i: d = 160 / DP = 160": (dict(C_=1280, heads=8, d=160, DP=160, tokens=256), 96, [77] * 3, GENERIC, [ATTN] * 3),
    "j: 96 tokens (a 12 x 8 grid)": (dict(L1280, tokens=96), 96, [77] * 3, GENERIC, [ATTN] * 3),
    "k: 960 tokens (24 x 40)": (dict(L1280, tokens=960), 96, [77] * 3, CROSS77, [C77] * 3),
}


@pytest.fixture
def ask(lib):
    """ask(layer, prompt_rows, key_counts, folded, recorded, debug bits) -> (kind, hand-over, stream kernels); the switches go back to 0."""
    def f(layer, rows, keys, folded=False, recorded=False, debug=0):
        lib.rt_op_gemm_debug(debug)
        try:
            return cross_route(prompt_rows=rows, key_counts=keys, folded=folded, recorded=recorded, lib=lib, **layer)
        finally:
            lib.rt_op_gemm_debug(0)
    return f


@pytest.mark.parametrize("name", list(ROWS))
def test_route_of_the_default_switches(ask, lib, name):
    layer, rows, keys, kind, kernels = ROWS[name]
    for folded in (False, True):
        for recorded in (False, True):
            got = ask(layer, rows, keys, folded, recorded)
            if lib.rt_op_probes_built() and not folded and not recorded and got[0] in (XATTN_FUSED, XBLOCK):
                continue                                     # (the one-launch forms of a probe build have their own test below)
            assert got[0] == kind and got[2] == kernels, (name, folded, recorded, got)
            assert got[1] == int(recorded and kind == CROSS77), (name, folded, recorded, got)      # hand-over: cross77_kernel of a recorded layer only


def test_handover_rows(ask):
    a, c, d = ROWS["a: 640 ch, 7 x 77 keys"], ROWS["c: 1280 ch, mixed counts"], ROWS["d: 1280 ch, all 77 in a 192-row cache"]
    assert ask(*a[:3], recorded=True)[:2] == (CROSS77, 1)
    assert ask(*a[:3], recorded=False)[:2] == (CROSS77, 0)
    assert ask(*a[:3], recorded=True, debug=B17)[:2] == (CROSS77, 0)       # row b: the store computes its own statistics, the route stays
    assert ask(*c[:3], recorded=True)[:2] == (RUNS, 0)
    # row d: the capacity does not change a 77-key launch
    for rows in (96, 192, 288):
        assert ask(d[0], rows, d[2], recorded=True) == (CROSS77, 1, [C77] * 4), rows


@pytest.mark.parametrize("name", list(ROWS))
def test_debug_bit_19_sends_everything_to_the_generic_kernel(ask, lib, name):
    layer, rows, keys, _, _ = ROWS[name]
    for recorded in (False, True):
        got = ask(layer, rows, keys, recorded=recorded, debug=B19 | B4)     # (bit 4: no fused to_q launch in a probe build either)
        assert got == (GENERIC, 0, [ATTN] * len(keys)), (name, got)
        if not lib.rt_op_probes_built():
            assert ask(layer, rows, keys, recorded=recorded, debug=B19) == got


@pytest.mark.parametrize("name", list(ROWS))
@pytest.mark.parametrize("debug", [0, B4, B16, B4 | B16, B19, B16 | B19])
def test_the_shipped_build_has_no_one_launch_form(ask, lib, name, debug):
    if lib.rt_op_probes_built():
        pytest.skip("a PROBES=1 build")
    layer, rows, keys, _, _ = ROWS[name]
    for folded in (False, True):
        assert ask(layer, rows, keys, folded, False, debug)[0] in (GENERIC, CROSS77, RUNS)


def test_refused_arguments(lib):
    def rc(rows, keys):
        k = C.c_int(-9)
        r = lib.rt_op_cross_route(640, 10, 64, 64, 4096, rows, (C.c_int * len(keys))(*keys) if keys else None, len(keys), 0, 0, C.byref(k), None, None)
        assert r == 0 or k.value == -9           # refused: nothing written
        return r
    assert rc(96, [77, 77]) == 0 and rc(192, [154, 77]) == 0 and rc(288, [231]) == 0
    for rows, keys in [(96, [76]), (96, [78]), (96, [154]), (192, [231]), (288, [308]), (96, [0]), (128, [77]), (96, []), (96, [77] * 17)]:
        assert rc(rows, keys) != 0, (rows, keys)


def test_one_launch_forms_of_a_probe_build(ask, lib):
    """PROBES=1 builds: xblock (debug bit 16) on the 640-channel level, the fused to_q launch (bit 4 clear) where cross77_kernel is off (bit
    19) and its tiling fits - both only with a 96-row cache, 77-key streams, no folded LayerNorm and no recorded map."""
    if not lib.rt_op_probes_built():
        pytest.skip("the shipped build has neither kernel")
    keys = [77] * 7
    assert ask(L640, 96, keys, debug=B16) == (XBLOCK, 0, [-1] * 7)
    assert ask(L640, 96, keys)[0] == CROSS77                                     # opt-in
    assert ask(L640, 96, keys, folded=True, debug=B16)[0] == CROSS77
    assert ask(L640, 96, keys, recorded=True, debug=B16)[:2] == (CROSS77, 1)
    assert ask(L640, 192, keys, debug=B16)[0] == CROSS77                         # the kernel holds the 96-row stride
    assert ask(L640, 192, [77, 154, 77], debug=B16)[0] == RUNS
    assert ask(dict(L640, tokens=960), 96, keys, debug=B16)[0] == CROSS77        # tokens % 128
    assert ask(L1280, 96, keys, debug=B16)[0] == CROSS77                         # 640 channels x 10 heads only
    assert ask(L640, 96, keys, debug=B16 | B19)[0] == XBLOCK                     # does not need cross77_kernel
    # fused to_q: (tokens / 128) (H 64 / 320) <= 40 tiles per stream - the 1280-channel level at 1024 tokens, not the 640-channel one at 4096
    assert ask(L1280, 96, keys, debug=B19) == (XATTN_FUSED, 0, [-1] * 7)
    assert ask(L1280, 96, keys)[0] == CROSS77                                    # cross77_kernel comes first
    assert ask(L1280, 96, keys, debug=B19 | B4)[0] == GENERIC
    assert ask(L1280, 96, keys, folded=True, debug=B19)[0] == GENERIC
    assert ask(L1280, 96, keys, recorded=True, debug=B19)[:2] == (GENERIC, 0)
    assert ask(L1280, 192, keys, debug=B19)[0] == GENERIC
    assert ask(L640, 96, keys, debug=B19)[0] == GENERIC
