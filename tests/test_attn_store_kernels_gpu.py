"""Every route of launch_attn_store (csrc/attn_store.hip) and the statistics hand-over from attn_kernel / cross77_kernel, per kernel
instantiation, against the fp64 softmax of tests/attn_store_ref.py.

Bar per element: |got - ref| <= A + R ref with A = 2^-23 and R = 16 R_control + NKpad 2^-23 (attn_store_ref.bar_R); R_control is what
the fp32 CPU control needs against the same reference - computed here from the reference, never from the device result.  Every case
prints the R it needed ("attn_store parity" lines; profiles/attn_store_parity.txt is that output)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import attn_store_ref as R  # noqa: E402
from hiputil import DEV, cross_route, probs_avg_rc, store_handover  # noqa: E402
from rich_text_to_image_amd.engine import load_library  # noqa: E402

GUARD = 4096                 # floats on either side of the output buffer
SENTINEL = -7777.25


class _debug:
    def __init__(self, bits):
        self.bits = bits

    def __enter__(self):
        load_library().rt_op_gemm_debug(self.bits)

    def __exit__(self, *exc):
        load_library().rt_op_gemm_debug(0)


def _guarded(N, NK, fill):
    big = torch.full((GUARD + N * NK + GUARD,), SENTINEL, device=DEV)
    out = big[GUARD:GUARD + N * NK].view(N, NK)
    out.fill_(fill)
    return big, out


def _guard_intact(big, N, NK):
    s = torch.tensor(SENTINEL, device=DEV)
    return bool((big[:GUARD] == s).all()) and bool((big[GUARD + N * NK:] == s).all())


def _ulp(x):
    return (torch.nextafter(x.abs(), torch.full_like(x, float("inf"))) - x.abs())


def _parity(tag, got, ref, Rbar, Rc):
    got = got.cpu()
    need, l2 = R.needed_R(got, ref, R.A_BAR), R.rel_l2(got, ref)
    print(f"attn_store parity {tag}: R needed {need:.3e}  bar R {Rbar:.3e} (R_control {Rc:.3e})  rel-L2 {l2:.3e}  rowsum err {(got.double().sum(-1) - 1).abs().max().item():.2e}")
    assert torch.isfinite(got).all(), tag
    assert Rbar <= 1e-3
    assert need <= Rbar, f"{tag}: needs R = {need:.3e} > bar {Rbar:.3e}"


def _semantics(tag, run, N, NK):
    """overwrite onto NaN, determinism, += twice, += onto a known buffer, guard band; returns the overwrite result.
    run(out, accumulate) launches the route under test."""
    big, out = _guarded(N, NK, float("nan"))
    run(out, 0)
    first = out.clone()
    assert torch.isfinite(first).all(), f"{tag}: overwrite left non-finite values"
    run(out, 1)
    twice = out.clone()
    assert _guard_intact(big, N, NK), f"{tag}: wrote outside [N, NK]"
    assert bool(((twice - 2 * first).abs() <= _ulp(2 * first)).all()), f"{tag}: accumulate != first + first"
    big2, out2 = _guarded(N, NK, float("nan"))
    run(out2, 0)
    assert torch.equal(out2, first), f"{tag}: two launches differ"
    base = 0.25 + 0.001 * torch.arange(N * NK, device=DEV, dtype=torch.float32).remainder(97).view(N, NK)
    out2.copy_(base)
    run(out2, 1)
    assert bool(((out2 - (base + first)).abs() <= _ulp(base + first)).all()), f"{tag}: accumulate does not add to the buffer"
    assert _guard_intact(big2, N, NK), f"{tag}: wrote outside [N, NK]"
    return first


_STORE_PARAMS = [(c[:6], name, bits, fam) for c in R.STORE_CASES for name, bits in c[6] for fam in R.FAMILIES]
_shown = set()               # routes whose discrimination control has been shown


@pytest.mark.parametrize("shape,route,bits,family", _STORE_PARAMS, ids=[f"{'x'.join(map(str, s))}-{n}-{f}" for s, n, _, f in _STORE_PARAMS])
def test_store_route_against_fp64_softmax(shape, route, bits, family):
    H, N, NK, NKpad, NKrows, d = shape
    DP = R.dp_of(d)
    key, (Qc, Kc) = R.store_operands(H, N, NK, NKpad, NKrows, d, family)
    show = route not in _shown and H > 1 and family == "plain"
    ref, Rc, Rbar, *wrong = R.reference(key, H, d, DP, NK, NKpad, show)
    # the operands sit behind a row offset, as a stream's rows do in the engine's buffers
    Q = torch.cat([torch.full((16, H * DP), 3.0, dtype=torch.bfloat16), Qc]).to(DEV)
    K = torch.cat([torch.full((32, H * DP), -3.0, dtype=torch.bfloat16), Kc]).to(DEV)
    tag = f"{route} H={H} N={N} NK={NK} NKpad={NKpad} d={d} {family}"

    def run(out, acc):
        rc = probs_avg_rc(Q, K, out, H, N, NK, NKpad, NKrows, DP, acc, q_row0=16, k_row0=32)
        assert rc == 0, load_library().rt_op_last_error().decode()
    with _debug(bits):
        got = _semantics(tag, run, N, NK)
    _parity(tag, got, ref, Rbar, Rc)
    if show:
        _shown.add(route)
        for name, w in zip(("head 0 instead of the head average", "key NK-1 dropped"), wrong):
            need = R.needed_R(w, ref, R.A_BAR)
            print(f"attn_store discrimination {route}: {name} needs R {need:.3e} = {need / Rbar:.0f} x the bar")
            assert need > 100 * Rbar


def _handover_self_inputs(H, N, d, family, B):
    DP = R.dp_of(d)
    qs, ks = [], []
    for b in range(B):
        q, k = R.make_qk(H, N, N, N, d, family, R.case_seed(H, N, d, b, R.FAMILIES.index(family)), self_attn=True)
        qs.append(R.pack_heads(q, H, d, DP, R.q_scale(d))); ks.append(R.pack_heads(k, H, d, DP))
    g = torch.Generator().manual_seed(R.case_seed(H, N, d))
    V = torch.randn(B * N, H * DP, generator=g).to(torch.bfloat16)
    return DP, qs, ks, torch.cat(qs).to(DEV), torch.cat(ks).to(DEV), V.t().contiguous().to(DEV)


def _takes_stats(N, DP):
    # attn_store_takes_stats as documented in include/rtdiff.h
    return 256 <= N <= 1024 and N % 32 == 0 and DP in (32, 64, 96)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("stream", [1, 2])
@pytest.mark.parametrize("H,N,d", R.HANDOVER_SELF)
def test_self_attention_statistics_handover(H, N, d, stream, family):
    """attn_kernel leaves (m, 1 / (H l)) of the recorded stream - m is a bf16 value, up to 8 below the row maximum (deferred rescale) -
    and the apply kernel alone rebuilds the map from it: same bar as the store's own statistics (bit 17), and O untouched by the side output."""
    B = R.HANDOVER_B
    DP, qs, ks, Q, K, VT = _handover_self_inputs(H, N, d, family, B)
    NKpad = (N + 31) // 32 * 32
    key = R.register(("self", H, N, d, family, stream), qs[stream], ks[stream])
    ref, Rc, Rbar = R.reference(key, H, d, DP, N, NKpad)
    res = {}
    for name, bits in (("hand-over", 0), ("own statistics", R.B17)):
        O = torch.zeros(B * N, H * DP, device=DEV, dtype=torch.bfloat16)
        taken = []
        tag = f"self {name} H={H} N={N} d={d} stream {stream} {family}"

        def run(out, acc):
            taken.append(store_handover(Q, K, VT, O, out, B, H, N, N, d, DP, stream, accumulate=acc))
        with _debug(bits):
            got = _semantics(tag, run, N, N)
        assert all(t == (bits == 0 and _takes_stats(N, DP)) for t in taken), (tag, taken)
        _parity(tag + (" [taken]" if taken[0] else " [not taken]"), got, ref, Rbar, Rc)
        res[name] = O
    assert torch.isfinite(res["hand-over"].float()).all()
    assert torch.equal(res["hand-over"], res["own statistics"]), "the statistics side output disturbed O"


def test_injected_recorded_stream_takes_no_handover():
    """q_src[b] != b: the attention launch computes another stream's softmax, so its statistics are not the recorded stream's."""
    H, N, d, B, stream, family = 1, 256, 32, R.HANDOVER_B, 2, "plain"
    DP, qs, ks, Q, K, VT = _handover_self_inputs(H, N, d, family, B)
    key = R.register(("self", H, N, d, family, stream), qs[stream], ks[stream])
    ref, Rc, Rbar = R.reference(key, H, d, DP, N, N)
    O = torch.zeros(B * N, H * DP, device=DEV, dtype=torch.bfloat16)
    big, out = _guarded(N, N, float("nan"))
    assert store_handover(Q, K, VT, O, out, B, H, N, N, d, DP, stream, qk_src=[0, 1, 1]) is False
    assert _guard_intact(big, N, N)
    _parity("self injected stream [not taken]", out, ref, Rbar, Rc)
    big, out = _guarded(N, N, float("nan"))
    assert store_handover(Q, K, VT, O, out, B, H, N, N, d, DP, stream, qk_src=[0, 1, 2]) is True
    _parity("self same inputs, own Q / K [taken]", out, ref, Rbar, Rc)


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("stream", [1, 2])
@pytest.mark.parametrize("H,N", R.HANDOVER_CROSS)
def test_cross77_statistics_handover(H, N, stream, family):
    """cross77_kernel leaves the statistics of the recorded stream, head (hg*HPW + h2); attn_store_apply2_kernel alone writes the
    [N, 77] map of the stream's PROMPT (k_row0 = prompt * 96; rows 77..95 hold anything finite)."""
    B, P, d, DP, KP = R.HANDOVER_B, 2, 64, 64, 96
    prompt = [1, 0, 1]
    assert prompt[stream] != stream
    qs, kp = [], [None] * P
    for b in range(B):
        q, k = R.make_qk(H, N, 77, KP, d, family, R.case_seed(H, N, b, R.FAMILIES.index(family)))
        qs.append(R.pack_heads(q, H, d, DP, R.q_scale(d)))
        if b >= 1:
            kp[prompt[b]] = R.pack_heads(k, H, d, DP)          # the spiked family's last valid key is made from a query of the stream that reads it
    g =torch.Generator().manual_seed(R.case_seed(H, N, 77))
    VT = torch.randn(H * DP, P * KP, generator=g).to(torch.bfloat16).to(DEV)
    Q, K = torch.cat(qs).to(DEV), torch.cat(kp).to(DEV)
    key = R.register(("cross", H, N, family, stream), qs[stream], kp[prompt[stream]])
    ref, Rc, Rbar = R.reference(key, H, d, DP, 77, KP)
    res = {}
    # bit 21: cross77_kernel's two-heads-per-workgroup form (statistics of head hg*2 + h2), which an even head count can take
    for name, bits in (("hand-over", 0), ("own statistics", R.B17)) + ((("hand-over, two heads per workgroup", 1 << 21),) if H % 2 == 0 else ()):
        O = torch.zeros(B * N, H * DP, device=DEV, dtype=torch.bfloat16)
        taken = []
        tag = f"cross {name} H={H} N={N} stream {stream} prompt {prompt[stream]} {family}"

        def run(out, acc):
            taken.append(store_handover(Q, K, VT, O, out, B, H, N, KP, d, DP, stream, cross=True, prompt=prompt, key_counts=[77] * B, accumulate=acc))
        with _debug(bits):
            got = _semantics(tag, run, N, 77)
            asked = cross_route(H * d, H, d, DP, N, KP, [77] * B, recorded=True)
        assert all(t == (bits != R.B17) for t in taken), (tag, taken)
        assert all(t == bool(asked[1]) for t in taken), (tag, taken, asked)      # the host-only query answers what the launch did
        _parity(tag + (" [taken]" if taken[0] else " [not taken]"), got, ref, Rbar, Rc)
        res[name] = O
    assert torch.isfinite(res["hand-over"].float()).all()
    assert torch.equal(res["hand-over"], res["own statistics"]), "the statistics side output disturbed O"
    if H % 2 == 0:
        assert torch.equal(res["hand-over"], res["hand-over, two heads per workgroup"])      # a query's bits do not depend on the grouping


@pytest.mark.parametrize("what,H,NK,NKpad,DP", [("NKpad % 32 != 0", 2, 77, 80, 64), ("H = 33", 33, 77, 96, 64), ("NK > NKpad", 2, 100, 96, 64),
                                               ("DP = 48", 2, 77, 96, 48)])
def test_store_refuses_shapes_outside_the_contract_on_the_host(what, H, NK, NKpad, DP):
    N = 32
    Q = torch.zeros(N, H * DP, device=DEV, dtype=torch.bfloat16)
    K = torch.zeros(128, H * DP, device=DEV, dtype=torch.bfloat16)
    big, out = _guarded(N, NK, 0.0)
    rc = probs_avg_rc(Q, K, out, H, N, NK, NKpad, 128, DP)
    msg = load_library().rt_op_last_error().decode()
    print(f"{what}: rc {rc}, '{msg}'")
    assert rc != 0 and "attn_store" in msg
    assert _guard_intact(big, N, NK) and bool((out == 0).all())


# ----------------------------------------------------------------------------------------------- SD-v1.5's head dims through the engine
SD_HEADDIM_CONFIG = dict(
    in_channels=4, out_channels=4, block_out_channels=(80, 160, 320, 320),
    down_block_types=("CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "CrossAttnDownBlock2D", "DownBlock2D"),
    up_block_types=("UpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D", "CrossAttnUpBlock2D"),
    layers_per_block=2, transformer_layers_per_block=(1, 1, 1, 1), attention_head_dim=(2, 2, 2, 2),
    cross_attention_dim=48, norm_num_groups=8, norm_eps=1e-5, use_linear_projection=False,
    addition_embed_type=None, addition_time_embed_dim=None, projection_class_embeddings_input_dim=None,
)


def test_plain_pass_records_maps_at_sd15_head_dims():
    """The plain pass of the SD facade on a UNet whose levels have SD-v1.5's head dims d = 40, 80, 160, 160 (DP = 64, 96, 160; two heads,
    a quarter of the width): 13 PLMS iterations of 12 requested steps on 64x64 latents.  EVERY row of the recorded self maps (32x32 at the
    d = 80 level: attn_kernel<96> hands its statistics to attn_store_apply_kernel<96>; 16x16 and 8x8 at d = 160: attn_store16_kernel<160>)
    and of the cross maps (attn_store16_kernel<96 | 160>; the module list records none at the d = 40 level) against the oracle's per-head probabilities of the text stream - method of tests/test_long_prompt_gpu.py, bounds of
    tests/test_attn_store_gpu.py (the trunk is fp16 / bf16 here: the fp32-class bar above does not apply)."""
    from oracle.schedulers import OraclePNDM
    from oracle.unet import OracleUNet, random_state_dict
    from rich_text_to_image_amd.attention_utils import CrossAttentionLayers, SelfAttentionLayers
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    cfg, sd = SD_HEADDIM_CONFIG, random_state_dict(SD_HEADDIM_CONFIG, seed=9)
    hw, steps, gs = 64, 12, 7.5
    g = torch.Generator().manual_seed(23)
    emb = torch.randn(2, 77, cfg["cross_attention_dim"], generator=g)
    lat0 = torch.randn(1, 4, hw, hw, generator=g)
    m = RegionDiffusion(0, unet_state_dict=sd, config=cfg)
    m.register_tokenmap_hooks()
    lat = m.plain_latents(emb, num_inference_steps=steps, guidance_scale=gs, latents=lat0.clone())
    o, sched = OracleUNet(cfg, sd), OraclePNDM()
    sched.set_timesteps(steps)
    acc, last, calls = {}, {}, {}

    def store(name, p, heads):
        calls[name] = calls.get(name, 0) + 1
        if calls[name] <= 10:                                        # rd.py:422
            return
        if name in SelfAttentionLayers and p.shape[1] <= 1024:
            last[name] = p.reshape(1, heads, p.shape[1], p.shape[2]).mean(1)              # rd.py:423: overwritten on every call
        elif name in CrossAttentionLayers:
            avg = p.reshape(1, heads, p.shape[1], p.shape[2]).mean(1)
            acc[name] = acc[name] + avg if name in acc else avg
    x = lat0.clone()
    with torch.no_grad():
        for t in sched.timesteps:
            eu = o.forward(x, t, emb[:1], None)
            et = o.forward(x, t, emb[1:2], None, store=store)
            x = sched.step(eu + gs * (et - eu), t, x)["prev_sample"]
    r = R.rel_l2(lat.cpu(), x.double())
    print(f"final latents rel-L2 {r:.3e}")
    assert r < 3e-2
    assert sum(v.shape[1] == 1024 for v in last.values()) >= 2 and len(acc) >= 4
    assert set(last) == set(m.selfattn_maps) and set(acc) == set(m.crossattn_maps)
    for k, ref in last.items():
        got = m.selfattn_maps[k].cpu()
        assert got.shape == ref.shape
        r, rs = R.rel_l2(got[0], ref[0].double()), (got[0].sum(-1) - ref[0].sum(-1)).abs().max().item()
        print(f"self {k} {list(ref.shape[1:])} every row: rel-L2 {r:.3e}, rowsum err {rs:.2e}")
        assert r < 3e-2 and rs < 2e-2 * ref[0].sum(-1).max().item()
    for k, ref in acc.items():
        got = m.crossattn_maps[k].cpu()
        assert got.shape == (1, ref.shape[1], 77)
        r, rs = R.rel_l2(got[0], ref[0].double()), (got[0].sum(-1) - ref[0].sum(-1)).abs().max().item()
        print(f"cross {k} [{ref.shape[1]}, 77] every row: rel-L2 {r:.3e}, rowsum err {rs:.2e}")
        assert r < 3e-2 and rs < 2e-2 * ref[0].sum(-1).max().item()
    m.remove_tokenmap_hooks()
    # the route of the d = 80 self layer, from the predicates the forward itself uses: rt_op_attention_store_handover at that layer's
    # shape (2 heads, 1024 tokens, DP 96; the text stream is stream 1 of 2 and attends with its own Q / K) reports the hand-over
    H, N, d, DP, B = 2, 1024, 80, 96, 2
    _, _, _, Q, K, VT = _handover_self_inputs(H, N, d, "plain", B)
    O = torch.zeros(B * N, H * DP, device=DEV, dtype=torch.bfloat16)
    big, out = _guarded(N, N, float("nan"))
    assert store_handover(Q, K, VT, O, out, B, H, N, N, d, DP, 1) is True
    assert _guard_intact(big, N, N) and torch.isfinite(out).all()
