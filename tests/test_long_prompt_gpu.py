"""Prompts longer than one 77-token CLIP window on the GPU: cross-attention over 154 / 231 keys with per-stream key counts
(csrc/attention.hip), the engine's K / V^T caches of 96 rows per window, rt_set_prompts_keys, the cross-map store and the facades.

A prompt of c windows has 77 c keys; a shorter prompt next to a longer one is NOT padded with empty windows: its rows behind its own
keys are masked.  The references below therefore run every stream over `emb[p, :count_p]` only."""
import ctypes as C
import math

import pytest
import torch

pytestmark = pytest.mark.gpu

from hiputil import DEV, _ptr, bf, chk, report  # noqa: E402
from test_kernels_gpu import _pack_heads, _ref_attention, rnd  # noqa: E402

GENERIC = 524288          # rt_op_gemm_debug bit 19: cross-attention on attn_kernel<CROSS> (the tile loop) for every shape


def attention_keys(Q, K, VT, B, H, N, NK, DP, prompt, counts, wset=None, wabs=None, wsgn=None):
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    O = torch.zeros(B * N, H * DP, device=DEV, dtype=torch.bfloat16)

    def ia(v):
        return (C.c_int * B)(*v) if v is not None else None
    chk(lib.rt_op_attention_keys(_ptr(Q), Q.stride(0), _ptr(K), K.stride(0), _ptr(VT), VT.stride(0), _ptr(O), O.stride(0), None,
                                 ia(prompt), ia(wset), _ptr(wabs), _ptr(wsgn), ia(counts), B, H, N, NK, DP, None))
    torch.cuda.synchronize()
    return O


# ----------------------------------------------------------------------------------------------- a. the kernels
WORD_POS = [2, 76, 77, 95, 96, 153, 191, 230]      # chunk seam 76|77, tile seams 95|96 and 191|192, last keys 153 and 230; 191 and 230 are
FONT_SIZE = [3.0, -1.5, 0.25, 0.0, -2.0, 20.0, 5.0, -0.5]                         # beyond the 154-key prompt: masked for its streams
COUNTS = [77, 154, 231]


def _long_inputs(B, H, N, d, DP):
    P, KP = 3, 288
    q = rnd(B, N, H * d, seed=160) * 3.0                                      # scores of a few units: a peaked softmax
    qs = d ** -0.5 * math.log2(math.e)
    Q = _pack_heads(q.reshape(B * N, -1), H, d, DP, qs)
    Kp = rnd(P, KP, H * d, seed=161) * 4.0                                    # finite junk in the rows behind a prompt's keys ...
    Vp = torch.full((P, KP, H * d), 7.0)                                      # ... and 7.0 in every padded V row: masked, not multiplied by ~0
    kc, vc = rnd(P, KP, H * d, seed=162), rnd(P, KP, H * d, seed=163)
    for p, c in enumerate(COUNTS):
        Kp[p, :c] = kc[p, :c]
        Vp[p, :c] = vc[p, :c]
    K = _pack_heads(Kp.reshape(P * KP, -1), H, d, DP)
    V = _pack_heads(Vp.reshape(P * KP, -1), H, d, DP)
    wabs, wsgn = torch.ones(2, KP), torch.ones(2, KP)                         # ones behind the keys too: the mask is the key count, not the table
    wp, fs = torch.tensor(WORD_POS), torch.tensor(FONT_SIZE)
    wabs[1, wp] = fs.abs(); wsgn[1, wp] = fs.sign()
    return Q, K, V, qs, wabs.to(DEV), wsgn.to(DEV)


def _check_long(B, H, N, d, DP, both_routes):
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    P, KP = 3, 288
    Q, K, V, qs, wabs, wsgn = _long_inputs(B, H, N, d, DP)
    prompt = [1, 2, 0, 2][:B]                                                 # streams use the prompts in mixed order
    counts = [COUNTS[p] for p in prompt]
    wset = [1, 1, -1, -1][:B]                                                 # font-size softmax on a 154-key and a 231-key stream
    VT = V.t().contiguous()
    out = attention_keys(Q, K, VT, B, H, N, KP, DP, prompt, counts, wset, wabs, wsgn)
    assert torch.isfinite(out.float()).all()
    qr = (Q.float() / qs).reshape(B, N, H, DP)[..., :d].reshape(B, N, H * d)
    kr = K.float().reshape(P, KP, H, DP)[..., :d].reshape(P, KP, H * d)
    vr = V.float().reshape(P, KP, H, DP)[..., :d].reshape(P, KP, H * d)
    got = out.float().reshape(B, N, H, DP)[..., :d].reshape(B, N, H * d)
    for b in range(B):
        c = counts[b]
        keep = [i for i, w in enumerate(WORD_POS) if w < c]                   # a position beyond the stream's keys has no effect
        fsz = (torch.tensor([WORD_POS[i] for i in keep]), torch.tensor([FONT_SIZE[i] for i in keep])) if wset[b] >= 0 else None
        ref, _ = _ref_attention(qr[b:b + 1], kr[prompt[b], :c][None], vr[prompt[b], :c][None], H, fsz)
        report(f"long cross d{d} B{B} H{H} N{N} stream {b} keys={c} fs={wset[b]}", got[b], ref[0], atol=2e-2, rtol=2e-2)
    if both_routes:
        lib.rt_op_gemm_debug(GENERIC)
        try:
            generic = attention_keys(Q, K, VT, B, H, N, KP, DP, prompt, counts, wset, wabs, wsgn)
        finally:
            lib.rt_op_gemm_debug(0)
        assert torch.isfinite(generic.float()).all()
        report("d = 64 route vs attn_kernel<CROSS>", out.float(), generic.float(), atol=2e-2, rtol=2e-2)
    return out


@pytest.mark.parametrize("B,H,N", [(4, 4, 256), (4, 5, 320)])
def test_long_cross_attention_d64_against_reference_arithmetic_and_the_generic_kernel(B, H, N):
    """The d = 64 shapes of SDXL through rt_op_attention_keys - the engine's route - and through the generic tile loop (debug bit 19),
    both against the reference processor's arithmetic in fp32 over each stream's OWN keys, and against each other.  On the engine's
    route the 77-key stream runs on cross77_kernel and the longer ones on crossmw_kernel (all their keys in LDS); behind bit 19 all
    four run in one launch of attn_kernel<CROSS>."""
    _check_long(B, H, N, 64, 64, both_routes=True)


@pytest.mark.parametrize("d,DP", [(32, 32), (160, 160)])
def test_long_cross_attention_generic_head_dims(d, DP):
    _check_long(4, 2, 256, d, DP, both_routes=False)


def test_a_77_key_stream_keeps_its_bits_next_to_longer_streams_and_in_a_wider_layout():
    """A prompt that fits one window attends over exactly its 77 keys whatever its neighbours are: the same bits alone in the 96-row
    layout of rt_op_attention, alone in the 288-row layout, and next to 154- and 231-key streams."""
    from hiputil import attention
    B, H, N, d, DP, KP = 4, 4, 256, 64, 64, 288
    Q, K, V, qs, wabs, wsgn = _long_inputs(B, H, N, d, DP)
    VT = V.t().contiguous()
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    lib.rt_op_gemm_debug(GENERIC)
    try:
        mixed = attention_keys(Q, K, VT, B, H, N, KP, DP, [1, 2, 0, 2], [154, 231, 77, 231], [1, 1, 1, -1], wabs, wsgn)
        alone = attention_keys(Q[2 * N:3 * N], K, VT, 1, H, N, KP, DP, [0], [77], [1], wabs, wsgn)
        K96, V96 = K[:96].contiguous(), V[:96].contiguous()
        w96a, w96s = wabs[:, :96].contiguous(), wsgn[:, :96].contiguous()
        w96a[:, 77:] = 0
        narrow = attention(Q[2 * N:3 * N], K96, V96.t().contiguous(), 1, H, N, 96, DP, k_src=[0], v_src=[0], cross=True, wabs=w96a,
                           wsgn=w96s, wset=[1], nk_valid=77)
    finally:
        lib.rt_op_gemm_debug(0)
    assert torch.equal(mixed[2 * N:3 * N], alone)
    assert torch.equal(alone, narrow)
    # ... and on the default route (cross77_kernel where every stream of the launch has 77 keys)
    mixed77 = attention_keys(Q, K, VT, B, H, N, KP, DP, [1, 2, 0, 2], [154, 231, 77, 231], [1, 1, 1, -1], wabs, wsgn)
    alone77 = attention_keys(Q[2 * N:3 * N], K, VT, 1, H, N, KP, DP, [0], [77], [1], wabs, wsgn)
    assert torch.equal(mixed77[2 * N:3 * N], alone77)
    # the long streams: crossmw_kernel here, attn_kernel<CROSS> above - the bound of the arithmetic class
    report("long streams, d = 64 route vs generic", torch.cat([mixed77[:2 * N], mixed77[3 * N:]]).float(),
           torch.cat([mixed[:2 * N], mixed[3 * N:]]).float(), atol=2e-2, rtol=2e-2)
    narrow77 = attention(Q[2 * N:3 * N], K96, V96.t().contiguous(), 1, H, N, 96, DP, k_src=[0], v_src=[0], cross=True, wabs=w96a,
                         wsgn=w96s, wset=[1], nk_valid=77)
    assert torch.equal(alone77, narrow77)


ONE_TILE = 1 << 20        # rt_op_gemm_debug bit 20: one 16-query tile per wave (cross77_kernel and crossmw_kernel)


def test_crossmw_tiling_never_changes_a_querys_bits():
    """crossmw_kernel gives a wave two 16-query tiles once the launch has 512 workgroups of 128 queries (cross77_kernel's rule) and one
    otherwise or behind debug bit 20: the same bits either way, for 154- and 231-key streams with and without the font-size softmax -
    and the shape at which the two-tile form runs agrees with the generic kernel."""
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    B, H, N, d, DP, KP = 4, 8, 2048, 64, 64, 288                              # (N / 128) B H = 512
    Q, K, V, qs, wabs, wsgn = _long_inputs(B, H, N, d, DP)
    VT = V.t().contiguous()
    args = (Q, K, VT, B, H, N, KP, DP, [1, 2, 2, 1], [154, 231, 231, 154], [1, 1, -1, -1], wabs, wsgn)
    two = attention_keys(*args)
    try:
        lib.rt_op_gemm_debug(ONE_TILE)
        one = attention_keys(*args)
        lib.rt_op_gemm_debug(GENERIC)
        generic = attention_keys(*args)
    finally:
        lib.rt_op_gemm_debug(0)
    assert torch.isfinite(two.float()).all()
    assert torch.equal(two, one)
    report("crossmw two-tile form vs attn_kernel<CROSS>", two.float(), generic.float(), atol=2e-2, rtol=2e-2)


@pytest.mark.parametrize("NK", [154, 231])
@pytest.mark.parametrize("d", [64, 80])
def test_attn_processor_takes_chunked_prompts(NK, d):
    """HipAttnProcessor with encoder_hidden_states of 77 c rows (every row a key), plain and with the font-size softmax on keys of the
    second / third window, against the reference processor's arithmetic in fp32.  d = 64 runs crossmw_kernel, d = 80 (padded to 96) the tile loop."""
    import torch.nn.functional as F
    from rich_text_to_image_amd.attention_processor import HipAttnProcessor
    from test_kernels_gpu import _StubAttention
    H, N, Dc, B = 2, 256, 96, 2
    C_ = H * d
    sd = {"to_q.weight": rnd(C_, C_, seed=1, scale=C_ ** -0.5), "to_k.weight": rnd(C_, Dc, seed=2, scale=Dc ** -0.5),
          "to_v.weight": rnd(C_, Dc, seed=3, scale=Dc ** -0.5), "to_out.0.weight": rnd(C_, C_, seed=4, scale=C_ ** -0.5), "to_out.0.bias": rnd(C_, seed=5)}
    x, ctx = rnd(B, N, C_, seed=6) * 2.0, rnd(B, NK, Dc, seed=7) * 2.0
    attn = _StubAttention(sd, H, cross_dim=Dc)
    proc = HipAttnProcessor()
    wp = torch.tensor([2, 76, 77, 120, 153] + ([154, 230] if NK == 231 else []))
    fs = torch.tensor([3.0, -1.5, 0.0, 20.0, -2.0] + ([0.25, 5.0] if NK == 231 else []))
    q, k, v = F.linear(x, sd["to_q.weight"]), F.linear(ctx, sd["to_k.weight"]), F.linear(ctx, sd["to_v.weight"])
    refs = {}
    for name, weights, fsz in (("plain", None, None), ("font-size", {"word_pos": wp, "font_size": fs}, (wp, fs))):
        y, maps = proc(attn, x.to(DEV), encoder_hidden_states=ctx.to(DEV), attn_weights=weights)
        o, _ = _ref_attention(q, k, v, H, fsz)
        refs[name] = ref = F.linear(o, sd["to_out.0.weight"], sd["to_out.0.bias"])
        assert torch.isfinite(y.float()).all()
        # four bf16 GEMMs around the bf16 attention against fp32: the class of the engine-level checks, the project's rel-L2 < 1.5e-2
        # (tests/test_engine_gpu.py) - the kernels' element-wise bound is test a's
        err = rel_l2(y.float().cpu(), ref)
        print(f"processor cross {NK} keys d{d} {name}: rel_l2={err:.4e}")
        assert err < 1.5e-2
        if weights is None:
            assert maps[0].shape == (B, N, NK)
    assert rel_l2(refs["font-size"], refs["plain"]) > 0.1                      # ... which the font sizes move by far more than the bound


# ----------------------------------------------------------------------------------------------- b - g. the engine
from oracle.schedulers import OracleEuler, OraclePNDM  # noqa: E402
from oracle.unet import INJECT_RESNET, TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict  # noqa: E402


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


def _engine(cfg, hw, sd, max_keys):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(cfg, hw, hw, device=0, max_streams=8, max_prompts=8, max_keys=max_keys)
    e.load_state_dict(sd)
    return e


@pytest.fixture(scope="module")
def engines():
    """per config: (cfg, weights, latent size, an engine built for three windows, a default engine) - built once, on first use"""
    made = {}

    def get(which):
        if which not in made:
            cfg, hw = (TINY_XL_CONFIG, 128) if which == "xl" else (TINY_SD_CONFIG, 64)      # the grids of test_engine_gpu.py
            sd = random_state_dict(cfg, seed=11)
            made[which] = (cfg, sd, hw, _engine(cfg, hw, sd, 231), _engine(cfg, hw, sd, 77))
        return made[which]
    yield get
    for v in made.values():
        v[3].close(); v[4].close()


def _stream_inputs(cfg, hw, xl, seed=123):
    g = torch.Generator().manual_seed(seed)
    D = cfg["cross_attention_dim"]
    emb = torch.randn(3, 154, D, generator=g)
    emb[:2, 77:] = 0                                      # prompts 0 (negative) and 1 (region) have one window: zero rows behind their keys
    pooled = torch.randn(3, 32, generator=g) if xl else None
    tid = torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]]) if xl else None
    lat, lat_ref = torch.randn(1, 4, hw, hw, generator=g), torch.randn(1, 4, hw, hw, generator=g)
    return emb, [77, 77, 154], pooled, tid, lat, lat_ref


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_batched_forward_with_mixed_key_counts_matches_oracle(which, engines, monkeypatch):
    """[uncond (77 keys), base (154 keys, font sizes on key 3 and on key 120 of the second window), text_ref (154), region (77,
    injected from text_ref)] in one batched launch, against the oracle run per stream over emb[p, :count_p]."""
    import long_prompt_ref
    import oracle.unet
    monkeypatch.setattr(oracle.unet, "attention_probs", long_prompt_ref.attention_probs)
    cfg, sd, hw, eng, _ = engines(which)
    xl = which == "xl"
    emb, counts, pooled, tid, lat, lat_ref = _stream_inputs(cfg, hw, xl)
    wp, fs = torch.tensor([3, 120]), torch.tensor([4.0, -2.0])
    o = OracleUNet(cfg, sd)

    def added(k):
        return {"text_embeds": pooled[k:k + 1], "time_ids": tid} if xl else None
    t = 701.0
    with torch.no_grad():
        r0 = o.forward(lat, t, emb[:1, :77], added(0))
        r1 = o.forward(lat, t, emb[2:3, :154], added(2), ctl={"fontsize": {"word_pos": wp, "font_size": fs}})
        cap = {}
        r2 = o.forward(lat_ref, t, emb[2:3, :154], added(2), ctl={"capture": cap})
        inj = {k: v for k, v in cap.items() if k.endswith("attn1") or k == INJECT_RESNET}
        r3 = o.forward(lat, t, emb[1:2, :77], added(1), ctl={"inject": inj})
    eng.set_prompts(emb.to(DEV), pooled.to(DEV) if xl else None, tid, key_counts=counts)
    eng.set_fontsize(wp, fs)
    x = torch.cat([lat, lat, lat_ref, lat]).to(DEV)
    out = eng.unet_forward(x, t, [0, 2, 2, 1], fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2])
    assert torch.isfinite(out).all()
    for name, got, ref in (("uncond", out[0], r0[0]), ("base+fontsize", out[1], r1[0]), ("text_ref", out[2], r2[0]),
                           ("region injected", out[3], r3[0])):
        r = rel_l2(got, ref)
        print(f"{which} long-prompt stream {name}: rel-L2 {r:.3e}")
        assert r < 1.5e-2, name
    plain = eng.unet_forward(x, t, [0, 2, 2, 1])
    assert rel_l2(plain[1], out[1]) > 1e-3 and rel_l2(plain[3], out[3]) > 1e-3          # the modes change the result
    alone = eng.unet_forward(x[:1], t, [0])
    assert rel_l2(alone[0], out[0]) < 1e-5                                               # batch invariance of the 77-key stream
    # the second window matters: the base stream over its first 77 keys only is another result
    eng.set_prompts(emb[:, :77].contiguous().to(DEV), pooled.to(DEV) if xl else None, tid)
    short = eng.unet_forward(x, t, [0, 2, 2, 1], fontsize=[0, 0, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2])
    assert rel_l2(short[2], out[2]) > 1e-3
    eng.set_fontsize(None, None)


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_capacity_does_not_change_a_77_key_forward(which, engines):
    """An engine built for 231 keys, given 77-key prompts, launches what a default engine launches (prompt stride as a parameter): same bits."""
    cfg, sd, hw, big, small = engines(which)
    xl = which == "xl"
    emb, _, pooled, tid, lat, lat_ref = _stream_inputs(cfg, hw, xl, seed=7)
    emb = emb[:, :77].contiguous()
    wp, fs = torch.tensor([3, 76]), torch.tensor([4.0, -2.0])
    x = torch.cat([lat, lat, lat_ref, lat]).to(DEV)
    outs = []
    for eng in (big, small):
        eng.set_prompts(emb.to(DEV), pooled.to(DEV) if xl else None, tid)
        eng.set_fontsize(wp, fs)
        outs.append(eng.unet_forward(x, 701.0, [0, 2, 2, 1], fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2]))
        eng.set_fontsize(None, None)
    assert torch.isfinite(outs[0]).all() and outs[0].abs().sum() > 0
    assert torch.equal(outs[0], outs[1])
    # ... and the same through rt_set_prompts_keys with every count 77 in a wider tensor
    wide = torch.cat([emb, torch.randn(3, 77, emb.shape[2])], 1)
    big.set_prompts(wide.to(DEV), pooled.to(DEV) if xl else None, tid, key_counts=[77, 77, 77])
    big.set_fontsize(wp, fs)
    again = big.unet_forward(x, 701.0, [0, 2, 2, 1], fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2])
    big.set_fontsize(None, None)
    assert torch.equal(again, outs[0])


def test_a_default_engine_refuses_long_prompts_and_stays_usable(engines):
    from rich_text_to_image_amd.engine import RtError
    cfg, sd, hw, _, small = engines("sd")
    emb, counts, _, _, lat, _ = _stream_inputs(cfg, hw, False)
    with pytest.raises(RtError) as ei:
        small.set_prompts(emb.to(DEV), key_counts=counts)
    assert ei.value.code == -1 and "154" in str(ei.value) and "77" in str(ei.value)          # RT_E_INVALID, both numbers named
    with pytest.raises(RtError):
        small.set_fontsize(torch.tensor([120]), torch.tensor([2.0]))                           # word_pos < max_keys
    small.set_prompts(emb[:, :77].contiguous().to(DEV))
    out = small.unet_forward(lat.to(DEV), 701.0, [1])
    assert torch.isfinite(out).all() and out.abs().sum() > 0
    for bad in ([77, 77, 100], [77, 77, 231]):                                                 # not whole windows / more than the tensor holds
        with pytest.raises(RtError):
            engines("sd")[3].set_prompts(emb.to(DEV), key_counts=bad)
    with pytest.raises(RtError):
        from rich_text_to_image_amd.engine import Engine
        Engine(cfg, hw, hw, device=0, max_keys=100)


def test_plain_pass_records_a_154_column_cross_map(monkeypatch):
    """Token maps of a two-window prompt: the plain pass of the SD facade (13 PLMS iterations of 12 requested steps, maps accumulated
    after a module's 10th call: rd.py:422) records [HW, 154] cross maps; against the oracle's per-head probabilities of the text stream
    averaged over heads and summed over the same calls - method and bound of tests/test_attn_store_gpu.py."""
    import long_prompt_ref
    import oracle.unet
    from rich_text_to_image_amd.attention_utils import CrossAttentionLayers
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    monkeypatch.setattr(oracle.unet, "attention_probs", long_prompt_ref.attention_probs)
    cfg, sd = TINY_SD_CONFIG, random_state_dict(TINY_SD_CONFIG, seed=5)
    hw, steps, gs = 64, 12, 7.5
    g = torch.Generator().manual_seed(17)
    emb = torch.randn(2, 154, cfg["cross_attention_dim"], generator=g)
    emb[0, 77:] = 0
    lat0 = torch.randn(1, 4, hw, hw, generator=g)
    m = RegionDiffusion(0, unet_state_dict=sd, config=cfg)
    m.register_tokenmap_hooks()
    lat = m.plain_latents((emb, [77, 154]), num_inference_steps=steps, guidance_scale=gs, latents=lat0.clone())
    # the oracle: one forward per stream and iteration (the streams have different key counts)
    o, sched = OracleUNet(cfg, sd), OraclePNDM()
    sched.set_timesteps(steps)
    acc, calls = {}, {}

    def store(name, p, heads):
        if not name.endswith("attn2"):
            return
        calls[name] = calls.get(name, 0) + 1
        if calls[name] > 10:
            avg = p.reshape(1, heads, p.shape[1], p.shape[2]).mean(1)
            acc[name] = acc[name] + avg if name in acc else avg
    x = lat0.clone()
    with torch.no_grad():
        for t in sched.timesteps:
            eu = o.forward(x, t, emb[:1, :77], None)
            et = o.forward(x, t, emb[1:2, :154], None, store=store)
            x = sched.step(eu + gs * (et - eu), t, x)["prev_sample"]
    assert rel_l2(lat, x) < 3e-2
    names = [n for n in CrossAttentionLayers if n in acc]
    assert len(names) >= 4
    for k in names:
        got = m.crossattn_maps[k].cpu()
        assert got.shape == (1, acc[k].shape[1], 154)
        r = rel_l2(got[0], acc[k][0])
        print(f"cross map {k} [{got.shape[1]}, 154]: rel-L2 {r:.3e}")
        assert r < 3e-2
        assert (got[0].sum(-1) - acc[k][0].sum(-1)).abs().max() < 2e-2 * acc[k][0].sum(-1).max()
    m.remove_tokenmap_hooks()


def test_facade_long_prompt_changes_the_image_and_rich_text_runs(tmp_path):
    """With max_prompt_chunks = 2 a word at token ~90 reaches the latents; with the default the text is cut at 75 tokens and cannot.
    A rich-text input whose size span sits behind token 75 runs through both passes."""
    import numpy as np
    from test_checkpoint_gpu import _write_dir
    from rich_text_to_image_amd.checkpoint import load_pipeline
    from rich_text_to_image_amd.sample import generate
    _write_dir(str(tmp_path))
    m = load_pipeline(str(tmp_path), "SD", device=0, latent_hw=(64, 64))
    head = " ".join(["sky"] * 88)
    a, b = head + " barn " + "sky sky", head + " fence " + "sky sky"                    # token 88 differs
    assert len(m.tokenizer._tokenize(a)) == 91
    lat = torch.randn(1, 4, 64, 64, generator=torch.Generator().manual_seed(0))
    m.masks = [torch.ones(1, 4, 64, 64)]

    def run(text, **kw):
        emb = m.get_text_embeds([text], [""], **kw)
        return m.produce_latents(emb, num_inference_steps=3, guidance_scale=7.5, latents=lat.clone())
    la, lb = run(a, max_prompt_chunks=2), run(b, max_prompt_chunks=2)
    assert torch.isfinite(la).all() and not torch.equal(la, lb) and rel_l2(la, lb) > 1e-4
    assert torch.equal(run(a), run(b))                                                  # default: the cut text cannot matter
    assert torch.equal(run(a, max_prompt_chunks=2), la)
    js = {"ops": [{"insert": "a "}, {"attributes": {"font": "slabo"}, "insert": "night sky"}, {"insert": " above " + head + " a "},
                  {"attributes": {"size": "60px"}, "insert": "barn"}, {"insert": " and a fence\n"}]}
    param = {"text_input": js, "height": 512, "width": 512, "guidance_weight": 7.5, "steps": 12, "noise_index": 1, "negative_prompt": "",
             "max_prompt_chunks": 2}
    plain, rich, _ = generate(m, param, "SD", None, inject_selfattn=0.3, num_segments=5, latents=lat.clone())
    assert plain.shape == rich.shape == (1, 512, 512, 3) and np.isfinite(rich.astype(np.float32)).all() and (rich != plain).any()
    with pytest.raises(ValueError, match="tokens"):                                     # three windows needed, two allowed: an error, not a cut
        generate(m, dict(param, text_input={"ops": [{"insert": " ".join(["sky"] * 160) + "\n"}]}), "SD", None, latents=lat.clone())


def test_region_step_with_a_154_key_base_prompt_is_hipgraph_capturable(engines):
    """tests/test_engine_gpu.py::test_region_step_is_hipgraph_capturable with a two-window base prompt: the multi-tile cross-attention
    launches of an injected step are captured and replay to the same bits."""
    import os
    cfg, sd, hw, eng, _ = engines("xl")
    g = torch.load(os.path.join(os.path.dirname(__file__), "golden", "tiny_xl_euler.pt"))
    inp, steps = g["inputs"], g["steps"]
    sched = OracleEuler(); sched.set_timesteps(steps)
    e77 = inp["embeds"]
    P = e77.shape[0]
    emb = torch.zeros(P, 154, e77.shape[2]); emb[:, :77] = e77
    emb[P - 1, 77:] = torch.randn(77, e77.shape[2], generator=torch.Generator().manual_seed(4))     # the base prompt's second window
    counts = [77] * (P - 1) + [154]
    eng.set_prompts(emb.to(DEV), inp["pooled"].to(DEV), inp["time_ids"], key_counts=counts)
    eng.set_masks(inp["masks"].repeat(1, 4, 1, 1).to(DEV))
    eng.set_fontsize(torch.tensor([3, 120]), torch.tensor([4.0, -2.0]))
    lat0 = (inp["latents"] * sched.init_noise_sigma).to(DEV)
    h = lat0.shape[2]

    def reset():
        eng.set_schedule(0, sched.timesteps.tolist(), sched.sigmas.tolist(), steps)
        eng.set_latents(lat0)
    reset()
    eng.region_step(0, g["guidance_scale"], g["inject_selfattn"], g["inject_background"], xl=True)
    eager = eng.read_latents(h, h).clone()
    assert torch.isfinite(eager).all()
    side = torch.cuda.Stream()
    eng.synchronize()
    eng.set_stream(side.cuda_stream)
    try:
        reset()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.region_step(0, g["guidance_scale"], g["inject_selfattn"], g["inject_background"], xl=True)
        for _ in range(2):
            reset()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(eng.read_latents(h, h), eager)
    finally:
        torch.cuda.synchronize()
        eng.set_stream(None)
    reset()
    eng.set_fontsize(None, None)
