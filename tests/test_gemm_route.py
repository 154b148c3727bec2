"""Host-only route queries (no GPU): rt_op_gemm_route answers for exactly the GemmArgs rt_op_gemm builds, rt_op_groupnorm_form from the
GroupNorm launcher's own predicate.  The case table of the memory-contract tests (tests/memcases.py) is evaluated through them: every case
takes the route it is listed under - with contiguous and with padded leading dimensions alike - and every (route, epilogue) pair that
exists behind the operator ABI has at least one case.  The VAE's hi / lo contraction (rt_op_gemm_hilo, HILO_CASES) likewise, through
rt_op_gemm_hilo_route: three launches over every single-pass route, and every one-launch form."""
import ctypes as C

import pytest

from memcases import (G16, G16_UP2, GEMM_CASES, HILO_CASES, HILO_FORMS, IMPLEMENTED, KIND_NAMES, KSPLIT, PATCH, PATCH_SPLIT, TILE, TRIPLE,
                      TRIPLE_ALL, TRIPLE_DENSE, TRIPLE_PATCH, UPCONV_CASES, case_id, hilo_id, hilo_route_args, route_args)
from rich_text_to_image_amd.engine import load_library


def route(lib, args):
    k, v, s = C.c_int(-9), C.c_int(-9), C.c_int(-9)
    assert lib.rt_op_gemm_route(*args, C.byref(k), C.byref(v), C.byref(s)) == 0, args
    return k.value, v.value, s.value


class switches:
    """rt_op_gemm_force_config / rt_op_gemm_debug for the duration of a case."""

    def __init__(self, lib, cfg, debug):
        self.lib, self.cfg, self.debug = lib, cfg, debug

    def __enter__(self):
        assert self.lib.rt_op_gemm_force_config(self.cfg) == 0
        self.lib.rt_op_gemm_debug(self.debug)

    def __exit__(self, *exc):
        self.lib.rt_op_gemm_force_config(-1)
        self.lib.rt_op_gemm_debug(0)


def test_kind_numbers_are_the_headers():
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rtdiff.h")).read()
    got = {m.group(1): int(m.group(2)) for m in re.finditer(r"RT_ROUTE_([A-Z0-9_]+) = (\d)", hdr)}
    assert got == {n: i for i, n in enumerate(KIND_NAMES)}


@pytest.mark.parametrize("case", GEMM_CASES, ids=case_id)
def test_case_takes_the_route_it_is_listed_under(case):
    lib = load_library()
    with switches(lib, case["cfg"], case["debug"]):
        plain, padded = route(lib, route_args(case)), route(lib, route_args(case, pad=8))
    assert plain == padded, "a leading dimension changed the route"
    assert plain[0] == case["kind"], f"{case_id(case)} takes {KIND_NAMES[plain[0]]}, slices {plain[2]}"
    if "var" in case:
        assert plain[1] == case["var"]
    if "slices" in case:
        assert plain[2] == case["slices"]
    assert (plain[2] > 1) == (case["kind"] in (KSPLIT, PATCH_SPLIT))


def test_every_route_and_epilogue_has_a_case():
    have = {(c["kind"], c["epi"]) for c in GEMM_CASES}
    have |= {(G16_UP2, 4) for u in UPCONV_CASES if u[6] == 1}
    want = {(k, e) for k, epis in IMPLEMENTED.items() for e in epis}
    # the hi / lo contraction (rt_op_gemm_hilo): TRIPLE over every single-pass route the VAE's shapes take, and every one-launch form
    have_hilo = {(c["kind"], c["pass_kind"]) for c in HILO_CASES}
    assert have_hilo == HILO_FORMS, sorted(HILO_FORMS ^ have_hilo)
    assert {p for k, p in HILO_FORMS if k == TRIPLE} == {TILE, KSPLIT, G16, PATCH} and {k for k, _ in HILO_FORMS if k != TRIPLE} == {G16, PATCH}
    for form in HILO_FORMS:                                           # each form with and without a residual; in place on both dense forms
        assert {bool(c["res"]) for c in HILO_CASES if (c["kind"], c["pass_kind"]) == form} == {False, True}, form
    assert {c["kind"] for c in HILO_CASES if c["res"] == "inplace"} == {G16, TRIPLE}
    assert any(c["pair"] for c in HILO_CASES) and any(not c["bias"] and not c["wact"] for c in HILO_CASES)
    assert {c["debug"] for c in HILO_CASES} == {0, TRIPLE_ALL, TRIPLE_PATCH, TRIPLE_DENSE}
    missing = sorted(want - have)
    assert not missing, [f"{KIND_NAMES[k]} epi {e}" for k, e in missing]
    assert {k for k, _ in have} == {TILE, G16, G16_UP2, PATCH, PATCH_SPLIT, KSPLIT}
    # all nine tile configurations, every reduction epilogue of both split forms
    assert {c["cfg"] for c in GEMM_CASES if c["kind"] == TILE and c["mode"] == 0} >= set(range(9))
    assert {c["epi"] for c in GEMM_CASES if c["kind"] == KSPLIT and c["mode"] == 0} == {0, 1, 2, 3, 4}


def hilo_route(lib, args):
    o = [C.c_int(-9) for _ in range(5)]
    assert lib.rt_op_gemm_hilo_route(*args, *[C.byref(x) for x in o]) == 0, args
    return tuple(x.value for x in o)                                   # kind, variant_or_cfg, slices, pass_kind, pair_ok


@pytest.mark.parametrize("case", HILO_CASES, ids=hilo_id)
def test_hilo_case_takes_the_route_it_is_listed_under(case):
    lib = load_library()
    with switches(lib, -1, case["debug"]):
        plain, padded = hilo_route(lib, hilo_route_args(case)), hilo_route(lib, hilo_route_args(case, pad=8))
        single = hilo_route(lib, hilo_route_args(case, hilo=False))
    assert plain == padded, "a leading dimension changed the route"
    kind, _, slices, pass_kind, pair_ok = plain
    assert (kind, pass_kind) == (case["kind"], case["pass_kind"]), f"{hilo_id(case)} takes {KIND_NAMES[kind]} over {KIND_NAMES[pass_kind]}, slices {slices}"
    assert (slices > 1) == (pass_kind == KSPLIT)
    # the pair output exists on the patch kernel's ONE launch only; the single-pass call (A_lo == NULL) takes the route of one TRIPLE pass
    assert pair_ok == int(kind == PATCH) and (not case["pair"] or pair_ok)
    assert single[0] == single[3] == pass_kind and single[2] == slices


def test_hilo_route_query_refuses_nonsense():
    lib = load_library()
    conv = (1, 0, 1, 7168, 136, 576, 0, 576, 136, 7168, 64, 112, 64, 64, 112)
    assert hilo_route(lib, conv)[0] == PATCH
    outs = [None] * 5
    assert lib.rt_op_gemm_hilo_route(*conv, *outs) == 0               # every output is optional
    k = C.c_int(-7)
    for bad in [(1, 0, 2) + conv[3:],                                  # stride 2 with symmetric padding: not a VAE mode
                (1, 0, 1, 7168 * 2) + conv[4:],                        # two images
                (1, 0, 1, 7168, 136, 584) + conv[6:],                  # K != 9 Cin
                (1, 1, 0, 300, 256, 256, 256, 256, 256, 0, 0, 0, 0, 0, 0),      # a dense pair output
                (1, 0, 0, 0, 256, 256, 256, 256, 256, 0, 0, 0, 0, 0, 0)]:
        assert lib.rt_op_gemm_hilo_route(*bad, C.byref(k), None, None, None, None) != 0 and k.value == -7, bad
    assert lib.rt_op_vae_groupnorm_nchunk(0) < 0
    # the VAE's chunk rule: HW / 128 rows clamped to [16, 128]
    assert [lib.rt_op_vae_groupnorm_nchunk(hw) for hw in (48, 50, 144, 200, 400, 2304, 16384, 1 << 20)] == [3, 4, 9, 13, 25, 128, 128, 8192]


def test_route_query_follows_the_switches_and_refuses_nonsense():
    lib = load_library()
    dense = (0, 1, 300, 200, 200, 200, 200, 200, 0, 0, 0, 0, 0, 0)
    assert route(lib, dense) == (TILE, 0, 1)
    with switches(lib, 3, 0):
        assert route(lib, dense) == (TILE, 3, 1)
    g16 = (0, 0, 300, 256, 256, 256, 256, 256, 0, 0, 0, 0, 0, 0)
    assert route(lib, g16)[0] == G16
    with switches(lib, -1, 2):                                         # bit 1: keep gemm16.hip out
        assert route(lib, g16)[0] == TILE
    ks = (0, 1, 72, 512, 512, 512, 512, 512, 0, 0, 0, 0, 0, 0)
    assert route(lib, ks) == (KSPLIT, -1, 2)
    with switches(lib, -1, 4):                                         # bit 2: no split-K
        assert route(lib, ks)[0] == TILE
    with switches(lib, 5, 0):                                          # a forced configuration does not change the split
        assert route(lib, ks) == (KSPLIT, -1, 2)
    # rt_op_gemm passes no stream shares: unlike rt_op_split_plan's answer for the engine's launch of the same 3 x 16 x 16 problem, which
    # also is the chunk split, a patch-eligible convolution that fills > 96 tiles stays whole on the patch kernel
    assert route(lib, (1, 4, 7168, 136, 576, 0, 576, 136, 7168, 64, 112, 64, 64, 112)) == (PATCH, -1, 1)
    assert route(lib, dense) == (TILE, 0, 1)
    k = C.c_int(-7)
    for bad in [(9,) + dense[1:], (0, 7) + dense[2:], (0, 1, 0) + dense[3:], (1, 1, 256, 64, 576, 0, 576, 64, 0, 16, 16, 64, 16, 16)]:
        assert lib.rt_op_gemm_route(*bad, C.byref(k), None, None) != 0 and k.value == -7
    assert lib.rt_op_gemm_route(*dense, None, None, None) == 0        # every output is optional


def test_groupnorm_form_query():
    lib = load_library()
    f = lib.rt_op_groupnorm_form
    # csrc/norm.hip gn_fused_vw: one launch while HW <= 1024, HW x channels per group <= 98304 and the group is loadable 4 / 8 wide
    assert f(2, 1280, 0, 32, 7, 1024) == 1 and f(2, 1280, 0, 32, 7, 1025) == 2
    assert f(2, 1280, 1280, 32, 3, 1008) == 1 and f(2, 2560, 1280, 32, 3, 1024) == 2          # 80 -> 120 channels per group: 122880 > 98304
    assert f(2, 320, 0, 32, 2, 96) == 2                                                          # 10 channels per group: no 4-wide loads
    assert f(0, 64, 0, 8, 2, 96) == 1 and f(1, 64, 0, 8, 2, 96) == 1
    assert {f(2, 640, 640, 32, b, 256) for b in (1, 2, 7)} == {1}                                # a function of ONE batch entry's shape
    lib.rt_op_gemm_debug(1 << 23)
    try:
        assert f(2, 1280, 0, 32, 7, 1024) == 2                                                   # bit 23: always two launches
    finally:
        lib.rt_op_gemm_debug(0)
    assert f(2, 1280, 0, 32, 7, 1024) == 1
    for bad in [(3, 64, 0, 8, 1, 64), (0, 0, 0, 8, 1, 64), (0, 64, 0, 7, 1, 64), (0, 64, 0, 8, 0, 64), (0, 64, 0, 8, 1, 0)]:
        assert f(*bad) < 0
