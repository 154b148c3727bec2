"""ControlNet on the GPU (csrc/control.hip, rt_set_control_hint / rt_set_control_scales / rt_op_control_add): the residual add against its
fp64 restatement at the derived bar with its memory contract and batch invariance, the hint embedder against its restatement, the forward
- every stream and every controlnet.* trace point - and the steps against tests/controlnet_ref.py, the split step, graph capture of
two steps, off-is-off against digests recorded on the commit before the ControlNet existed, the refusals and the facade."""
import functools
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import controlnet_ref as R  # noqa: E402
from freeu_ref import FORWARD_BAR, oracle_streams, rel_l2  # noqa: E402
from memguard import damage, guarded, intact, poisoned  # noqa: E402
from oracle.region_loop import rich_step_forwards  # noqa: E402
from oracle.unet import OracleUNet  # noqa: E402

DEV = "cuda:0"
STEP_BAR = 3e-2                  # latent UPDATE of one step against the composition of oracle forwards (tests/test_nonsquare_gpu.py)
CN = dict(embed_channels=R.TINY_EMBED)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "controlnet_off_bits.json")


# ---------------------------------------------------------------------------------------------------------------- the add
ADD_STREAMS = lambda B: [0, B - 1]              # noqa: E731  a skipped stream (or several) in the middle
ADD_SCALES = [0.6, -0.5]


def _add(skip, r, streams, scales, lds=None, ldr=None, guard=False):
    """The op on CPU tensors skip fp16 [B, HW, C], r fp32 [n, HW, C] with leading dimensions lds / ldr (default C); guard: skip in a
    guarded window, r poisoned (tests/memguard.py).  Returns (skip after, on the CPU; (big, window))."""
    from rich_text_to_image_amd.engine import control_add
    B, HW, C = skip.shape
    n = r.shape[0]
    lds, ldr = lds or C, ldr or C
    if guard:
        big, sw = guarded((B * HW, C), torch.float16, lds, fill="bytes", device=DEV)
        sw.copy_(skip.reshape(B * HW, C))
        rw = poisoned(r.reshape(n * HW, C).to(DEV), ldr)
    else:
        def wide(t, ld):
            buf = torch.full((t.shape[0], ld), float("nan"), dtype=t.dtype, device=DEV)
            buf[:, :t.shape[1]] = t
            return buf[:, :t.shape[1]]
        sw, rw, big = wide(skip.reshape(B * HW, C), lds), wide(r.reshape(n * HW, C), ldr), None
    sv = torch.as_strided(sw, (B, HW, C), (HW * lds, lds, 1), sw.storage_offset())
    rv = torch.as_strided(rw, (n, HW, C), (HW * ldr, ldr, 1), rw.storage_offset())
    control_add(sv, rv, streams, scales)
    return sv.cpu(), (big, sw)


@pytest.mark.parametrize("B,HW,C", R.ADD_CASES, ids=[f"B{b}-HW{n}-C{c}" for b, n, c in R.ADD_CASES])
def test_add_matches_the_fp64_restatement(B, HW, C):
    """Every element within one fp32 rounding of the fma plus one fp16 rounding of skip + scale r in fp64; leading dimensions wider than
    C, the streams in the middle skipped (they keep their bytes), scales 0.6 and -0.5; a second launch on the same inputs gives the same
    bits."""
    skip, r = R.add_inputs(B, HW, C, 2)
    streams = ADD_STREAMS(B)
    got, _ = _add(skip, r, streams, ADD_SCALES, lds=C + 8, ldr=C + 4)
    ref, bar = R.add_ref(skip, r, streams, ADD_SCALES)
    err = (got.double() - ref).abs()
    worst = float((err / bar.clamp_min(1e-300))[streams].max())
    print(f"control_add B {B} HW {HW} C {C}: worst |got - ref| / bar = {worst:.3f}")
    assert bool(torch.isfinite(got.float()).all())
    assert bool((err <= bar).all()), worst
    for b in range(B):
        if b not in streams:
            assert torch.equal(got[b].view(torch.int16), skip[b].view(torch.int16)), b
    for i, b in enumerate(streams):
        assert float(((skip[b].double() - ref[b]).abs() > bar[b]).double().mean()) > 0.9       # the input itself (a dropped add) is far outside
    again, _ = _add(skip, r, streams, ADD_SCALES, lds=C + 8, ldr=C + 4)
    assert torch.equal(again.view(torch.int16), got.view(torch.int16))


@pytest.mark.parametrize("B,HW,C", R.ADD_CASES, ids=[f"B{b}-HW{n}-C{c}" for b, n, c in R.ADD_CASES])
def test_add_memory_contract_and_batch_invariance(B, HW, C):
    """skip in a guarded window, r poisoned: the guards and the padding columns of skip keep their bytes, the NaN padding of r is never
    read, the skipped streams keep their bytes; and a stream launched alone equals the same stream of the launch of several, bit for bit."""
    skip, r = R.add_inputs(B, HW, C, 2, seed=1)
    streams = ADD_STREAMS(B)
    got, (big, sw) = _add(skip, r, streams, ADD_SCALES, lds=C + 24, ldr=C + 12, guard=True)
    assert intact(big, sw), damage(big, sw)
    assert bool(torch.isfinite(got.float()).all())
    ref, bar = R.add_ref(skip, r, streams, ADD_SCALES)
    assert bool(((got.double() - ref).abs() <= bar).all())
    for b in range(B):
        if b not in streams:
            assert torch.equal(got[b].view(torch.int16), skip[b].view(torch.int16)), b
    for i, b in enumerate(streams):
        one, _ = _add(skip[b:b + 1], r[i:i + 1], [0], ADD_SCALES[i:i + 1])
        assert torch.equal(one[0].view(torch.int16), got[b].view(torch.int16)), b
    if B >= 3:                            # the launch order is the caller's: entry 0 may name the last stream
        rev, _ = _add(skip, r.flip(0), streams[::-1], ADD_SCALES[::-1])
        assert torch.equal(rev.view(torch.int16), got.view(torch.int16))


def test_add_refuses_what_it_cannot_do():
    from rich_text_to_image_amd.engine import RtError
    skip, r = R.add_inputs(3, 8, 16, 2)
    for kw in (dict(streams=[0, 3]), dict(streams=[1, 1]), dict(streams=[-1, 0]), dict(scales=[float("nan"), 1.0]), dict(scales=[1.0, float("inf")]),
               dict(lds=20), dict(ldr=18)):
        a = dict(streams=[0, 2], scales=ADD_SCALES)
        a.update(kw)
        with pytest.raises(RtError) as e:
            _add(skip, r, a.pop("streams"), a.pop("scales"), **a)
        assert e.value.code == -1, kw
    with pytest.raises(RtError):
        _add(skip[..., :12], r[..., :12], [0, 2], ADD_SCALES)                 # C % 8


# ---------------------------------------------------------------------------------------------------------------- engines
def _engine(cfg, h, w, sd, **kw):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(cfg, h, w, device=0, **kw)
    e.load_state_dict(sd)
    assert e.weights_missing()[0] == 0
    return e


def _set_prompts(eng, c):
    if c["xl"]:
        eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
    else:
        eng.set_prompts(c["emb"].to(DEV))
    eng.set_fontsize(c["wp"], c["fs"])


def _forward(eng, c, trace=None):
    x = torch.cat([c["lat"], c["lat"], c["lat_ref"], c["lat"]]).to(DEV)
    out = eng.unet_forward(x, c["t"], [0, 2, 2, 1], fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2], trace=trace)
    return (out[0].cpu(), out[1].cpu()) if trace else out.cpu()


# ---------------------------------------------------------------------------------------------------------------- the embedder
@pytest.mark.parametrize("h,w", [(16, 24), (32, 64)], ids=["3x128x192", "3x256x512"])
def test_embedder_matches_its_restatement(h, w):
    """control_embedding() against the exact fp64 restatement at the bar derived in tests/controlnet_ref.py (margin x the error of an
    emulation that rounds where an honest kernel does); the same bits on a second call and after set_prompts."""
    c = R.control_case("xl")
    hint = R.make_hint(h, w, seed=9)
    eng = _engine(c["cfg"], 32, 64, c["sd_cn"], controlnet=CN)
    try:
        assert eng.control_embedding() is None
        eng.set_control_hint(hint.to(DEV))
        got = eng.control_embedding().cpu()
        exact = R.embed_ref(c["cn"], hint).permute(1, 2, 0).reshape(h * w, -1)
        assert tuple(got.shape) == tuple(exact.shape)
        bar = R.embed_bar(c["cn"], hint)
        d = rel_l2(got, exact)
        print(f"hint embedder {8 * h} x {8 * w}: rel-L2 vs the exact restatement {d:.3e}, bar {bar:.3e}")
        assert bool(torch.isfinite(got).all())
        assert d <= bar
        eng.set_control_hint(hint.to(DEV))
        assert torch.equal(eng.control_embedding().cpu(), got)
        _set_prompts(eng, c)
        assert torch.equal(eng.control_embedding().cpu(), got)                   # the hint survives set_prompts
        eng.set_control_hint(None)
        assert eng.control_embedding() is None
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- the forward
@functools.lru_cache(maxsize=None)
def _forward_refs(which):
    c = R.control_case(which)
    outs, tr = R.traced_streams(R.ControlOracleUNet(c["cfg"], c["sd"], c["cn"], c["hint"], R.FORWARD_STREAM_SCALES), c)
    return c, outs, tr


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_forward_with_stream_modes_matches_the_control_ref(which):
    """One batched forward of uncond / base + font size / text_ref / injected region with the scales base 1.0 / region 0.5 / uncond 0:
    every stream within the project's forward bar of the ref; the uncontrolled stream bit-equal to the same forward on an engine without
    a ControlNet; a controlled stream run alone equals itself in the batch, bit for bit."""
    c, ref, _ = _forward_refs(which)
    eng = _engine(c["cfg"], c["h"], c["w"], c["sd_cn"], controlnet=CN)
    plain = _engine(c["cfg"], c["h"], c["w"], c["sd"])
    try:
        _set_prompts(eng, c); _set_prompts(plain, c)
        eng.set_control_hint(c["hint"].to(DEV))
        eng.set_control_scales(R.FORWARD_SLOT_SCALES)
        got, off = _forward(eng, c), _forward(plain, c)
        for k, name in enumerate(("uncond", "base+fontsize", "text_ref", "region injected")):
            r = rel_l2(got[k], ref[k])
            print(f"{which} stream {name}: rel-L2 vs the control ref {r:.3e}; vs the engine without a ControlNet {rel_l2(got[k], off[k]):.3e}")
            assert r < FORWARD_BAR, name
        assert torch.equal(got[0], off[0])
        assert all(rel_l2(got[k], off[k]) > 5 * FORWARD_BAR for k in (1, 2, 3))
        alone = eng.unet_forward(c["lat"].to(DEV), c["t"], [2], fontsize=[1]).cpu()
        assert torch.equal(alone[0], got[1])
        assert torch.equal(_forward(eng, c), got)
    finally:
        eng.close(); plain.close()


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_every_controlnet_trace_point_matches_the_ref(which):
    """rt_unet_forward_trace on every controlnet.* module: the control copy's modules (the controlled streams 1, 2, 3 in stream order), the
    hint embedding, and the main UNet's skips / mid output after the add (all four streams; the uncontrolled one is the un-added
    tensor), each within the forward bar of the ref's trace; the traced forward's output keeps its bits.

    (MI355X: worst point 1.43e-2 on [sd] - the control copy's deepest module, controlnet.mid_block.resnets.1, on a 4 x 8 grid - and 1.08e-2 on
    [xl]; the distance grows module by module as the main trunk's does, 1.0e-3 at controlnet.conv_in.  With the embedder on bf16 operands
    the same point was 1.56e-2: the embedder runs in fp32 for that reason, csrc/control.hip.)"""
    c, _, tr = _forward_refs(which)
    src = R.skip_sources(c["cfg"])
    eng = _engine(c["cfg"], c["h"], c["w"], c["sd_cn"], controlnet=CN)
    try:
        _set_prompts(eng, c)
        eng.set_control_hint(c["hint"].to(DEV))
        eng.set_control_scales(R.FORWARD_SLOT_SCALES)
        want_out = _forward(eng, c)
        names = [n for n, _, _ in eng.trace_modules() if n.startswith("controlnet.")]
        assert len(names) > len(src) + 5
        worst = (0.0, None)
        for name in names:
            out, t = _forward(eng, c, trace=name)
            assert torch.equal(out, want_out), name
            if name == "controlnet.hint_embedding":
                pairs = [(t[0], tr[1][name][0])]
                assert bool(torch.isnan(t[1:]).all())
            elif name.startswith("controlnet.skip.") or name == "controlnet.mid":
                un = src[int(name.rsplit(".", 1)[1])] if name != "controlnet.mid" else "mid_block.resnets.1"
                pairs = [(t[0], tr[0][un][0])] + [(t[k], tr[k][name][0]) for k in (1, 2, 3)]
            else:
                pairs = [(t[k - 1], tr[k][name][0]) for k in (1, 2, 3)]
                assert bool(torch.isnan(t[3]).all())
            for got, want in pairs:
                assert tuple(got.shape) == tuple(want.shape), name
                d = rel_l2(got, want)
                worst = max(worst, (d, name))
                assert d < FORWARD_BAR, (name, d)
        print(f"{which}: {len(names)} controlnet.* trace points, worst rel-L2 {worst[0]:.3e} at {worst[1]}")
        # with no stream controlled the main-side points read the un-added tensors and the control copy's modules are refused
        from rich_text_to_image_amd.engine import RtError
        eng.set_control_scales([0.0, 0.0, 0.0])
        _, t = _forward(eng, c, trace="controlnet.skip.1")
        assert rel_l2(t[1], tr[1][src[1]][0]) < FORWARD_BAR
        with pytest.raises(RtError) as e:
            _forward(eng, c, trace="controlnet.mid_block.resnets.1")
        assert e.value.code == -1
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- steps
def _rich_setup(eng, c, control=True):
    eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
    eng.set_masks(c["masks"].to(DEV))
    eng.set_fontsize(torch.tensor([3, 5]), torch.tensor([4.0, -2.0]))
    if control:
        eng.set_control_hint(c["hint"].to(DEV))
        eng.set_control_scales(R.STEP_SLOT_SCALES)


def _rich_reset(eng, c):
    eng.set_schedule(0, c["sched"].timesteps.tolist(), c["sched"].sigmas.tolist(), c["steps"])
    eng.set_latents(c["lat"].to(DEV))


@pytest.fixture(scope="module")
def rich():
    c = R.rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd_cn"], controlnet=CN)
    _rich_setup(eng, c)
    yield c, eng
    eng.close()


def test_region_step_matches_the_composition_of_control_ref_forwards(rich):
    """The injected first region_step (6 streams: uncond, base, uncond_ref, text_ref, two regions) with scales negative 0.7 / region 0 0.5 / region 1 off / base 1.0: both latent streams after the scheduler step against
    rich_step_forwards on the control ref, on the latent UPDATE; the plain oracle is far away."""
    c, eng = rich
    R_ = c["masks"].shape[0]
    _rich_reset(eng, c)
    eng.region_step(0, c["gs"], c["isa"], 0.0, xl=True)
    got, got_ref = (t.cpu() for t in eng.read_latents(c["hw"], c["hw"], with_ref=True))
    sched, lat0, gs = c["sched"], c["lat"], c["gs"]
    t = sched.timesteps[0]
    assert float(t) > (1 - c["isa"]) * 1000
    s = R.STEP_SLOT_SCALES
    # forwards of rich_step_forwards: uncond (slot 0), base (R), uncond_ref (0), text_ref (R), regions (1 .. R - 1)
    o = R.ControlOracleUNet(c["cfg"], c["sd"], c["cn"], c["hint"], [s[0], s[R_], s[0], s[R_]] + [s[k] for k in range(1, R_)])

    def added_fn(k):
        k = k if k >= 0 else c["pooled"].shape[0] + k
        return {"text_embeds": c["pooled"][k:k + 1], "time_ids": c["tid"]}
    lat_in = sched.scale_model_input(lat0, t)
    tfd = {"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])}
    masks = [c["masks"][r:r + 1] for r in range(R_)]

    def compose(unet):
        eu, et, eur, etr = rich_step_forwards(unet, lat_in, lat_in.clone(), t, c["emb"], added_fn, masks, tfd, True, True)
        out = sched.step(torch.cat([eu + gs * (et - eu), eur + gs * (etr - eur)]), t, torch.cat([lat0, lat0]))["prev_sample"]
        return torch.chunk(out, 2, dim=0)
    ref, ref_ref = compose(o)
    pl, pl_ref = compose(OracleUNet(c["cfg"], c["sd"]))
    r, rr = rel_l2(got - lat0, ref - lat0), rel_l2(got_ref - lat0, ref_ref - lat0)
    d, dr = rel_l2(pl - lat0, ref - lat0), rel_l2(pl_ref - lat0, ref_ref - lat0)
    print(f"region_step with a ControlNet: latent UPDATE rel-L2 {r:.3e} (reference stream {rr:.3e}); the oracle without control is {d:.3e} / {dr:.3e} away")
    assert r < STEP_BAR and rr < STEP_BAR
    assert d > 3 * STEP_BAR and dr > 3 * STEP_BAR


def test_plain_step_matches_the_composition_of_control_ref_forwards():
    """plain_step (streams [uncond = slot 0, text = slot 1]) with scales 0.7 / 1.0."""
    c = R.rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd_cn"], controlnet=CN)
    try:
        emb, pooled = c["emb"][[0, 3]], c["pooled"][[0, 3]]
        eng.set_prompts(emb.to(DEV), pooled.to(DEV), c["tid"])
        eng.set_control_hint(c["hint"].to(DEV))
        eng.set_control_scales([0.7, 1.0])
        _rich_reset(eng, c)
        eng.plain_step(0, c["gs"])
        got = eng.read_latents(c["hw"], c["hw"]).cpu()
    finally:
        eng.close()
    sched, lat0, gs = c["sched"], c["lat"], c["gs"]
    t = sched.timesteps[0]
    x = sched.scale_model_input(lat0, t)

    def compose(unet):
        with torch.no_grad():
            eu = unet.forward(x, t, emb[:1], {"text_embeds": pooled[:1], "time_ids": c["tid"]})
            et = unet.forward(x, t, emb[1:], {"text_embeds": pooled[1:], "time_ids": c["tid"]})
        return sched.step(eu + gs * (et - eu), t, lat0)["prev_sample"]
    ref = compose(R.ControlOracleUNet(c["cfg"], c["sd"], c["cn"], c["hint"], [0.7, 1.0]))
    pl = compose(OracleUNet(c["cfg"], c["sd"]))
    r, d = rel_l2(got - lat0, ref - lat0), rel_l2(pl - lat0, ref - lat0)
    print(f"plain_step with a ControlNet: latent UPDATE rel-L2 {r:.3e}; the oracle without control is {d:.3e} away")
    assert r < STEP_BAR
    assert d > 3 * STEP_BAR


def test_split_step_equals_the_whole_step_with_a_controlnet(rich):
    """rt_region_step_part for both parts of two, then _finish, gives the bits of rt_region_step (and likewise the plain step): a stream is
    controlled by the scale of the prompt it runs, whichever rank runs it."""
    c, eng = rich
    for i in (0, c["steps"] - 1):
        _rich_reset(eng, c)
        eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=True)
        whole = eng.read_latents(c["hw"], c["hw"], with_ref=True)
        _rich_reset(eng, c)
        ranges = [eng.region_step_part(i, c["gs"], c["isa"], c["ibg"], True, part, 2)[:2] for part in (0, 1)]
        assert all(n > 0 for _, n in ranges), ranges
        eng.region_step_finish(i, c["gs"], c["isa"], c["ibg"], True)
        parts = eng.read_latents(c["hw"], c["hw"], with_ref=True)
        assert torch.equal(parts[0], whole[0]) and torch.equal(parts[1], whole[1]), i
    _rich_reset(eng, c)
    eng.plain_step(0, c["gs"])
    whole = eng.read_latents(c["hw"], c["hw"])
    _rich_reset(eng, c)
    for part in (0, 1):
        eng.plain_step_part(0, part, 2)
    eng.plain_step_finish(0, c["gs"])
    assert torch.equal(eng.read_latents(c["hw"], c["hw"]), whole)


def test_two_region_steps_with_a_controlnet_are_hipgraph_capturable(rich):
    """As test_region_step_is_hipgraph_capturable (tests/test_engine_gpu.py) with control on, over TWO steps: nothing is allocated and
    nothing synchronises inside a step - either would end the capture with an error - (streams and scales travel in the kernel
    arguments), and the replay gives the eager steps' bits."""
    c, eng = rich
    hw = c["hw"]

    def two_steps():
        eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
        eng.region_step(1, c["gs"], c["isa"], c["ibg"], xl=True)
    _rich_reset(eng, c)
    two_steps()
    eager = eng.read_latents(hw, hw).clone()
    side = torch.cuda.Stream()
    eng.synchronize()
    eng.set_stream(side.cuda_stream)
    try:
        _rich_reset(eng, c)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            two_steps()
        for _ in range(2):
            _rich_reset(eng, c)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(eng.read_latents(hw, hw), eager)
    finally:
        torch.cuda.synchronize()
        eng.set_stream(None)
    _rich_reset(eng, c)


def test_the_add_is_profiled_under_its_own_class(rich):
    c, eng = rich
    _rich_reset(eng, c)
    eng.profile_enable(True)
    eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
    eng.synchronize()
    p = eng.profile_read_control()
    eng.profile_enable(False)
    assert p["launches"] == len(R.skip_channels(c["cfg"])) + 1 and p["total_bytes"] > 0 and p["total_ms"] > 0 and p["total_flops"] == 0, p


# ---------------------------------------------------------------------------------------------------------------- off is off
def test_off_is_off_against_the_bits_of_the_commit_before():
    """tests/golden/controlnet_off_bits.json holds the sha256 of the tiny forwards and of one region step, recorded on the GPU by
    controlnet_ref.off_digests on the commit before the ControlNet existed.  This tree reproduces them with no ControlNet, with one
    loaded but no hint, and with a hint but all scales 0."""
    with open(GOLDEN) as f:
        want = json.load(f)["digests"]

    def with_cn(cfg, h, w, sd):
        cn = R.control_state_dict(cfg, seed=21)
        return _engine(cfg, h, w, {**sd, **R.prefixed(cn)}, controlnet=CN)

    def hint_and_zero_scales(eng, c):
        eng.set_control_hint(R.make_hint(c["h"], c["w"]).to(DEV))
        eng.set_control_scales([0.0] * c["emb"].shape[0])
    assert R.off_digests(lambda cfg, h, w, sd: _engine(cfg, h, w, sd)) == want
    assert R.off_digests(with_cn) == want
    assert R.off_digests(with_cn, hint_and_zero_scales) == want


# ---------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_leave_the_engine_usable(rich):
    """RT_E_INVALID for a forward whose size differs from the hint's, a non-finite scale, too many scales, and every control call on an
    engine without a ControlNet; the state is unchanged: the next forward keeps its bits."""
    from rich_text_to_image_amd.engine import RtError
    import ctypes as C
    c, eng = rich
    x = c["lat"].to(DEV)
    before = eng.unet_forward(x, 500.0, [3]).cpu()
    for bad in ([0.7, float("nan"), 0.0, 1.0], [0.7, 0.5, float("inf"), 1.0], list(R.STEP_SLOT_SCALES) + [1.0], []):
        with pytest.raises(RtError) as e:
            eng.set_control_scales(bad)
        assert e.value.code == -1, bad
        assert torch.equal(eng.unet_forward(x, 500.0, [3]).cpu(), before)
    assert eng.lib.rt_set_control_scales(eng.h, None, 4) == -1
    half = c["hw"] // 2
    with pytest.raises(RtError) as e:                                            # the hint is 32 x 32, the forward 16 x 16
        eng.unet_forward(x[..., :half, :half].contiguous(), 500.0, [3])
    assert e.value.code == -1 and "never resized" in str(e.value)
    assert torch.equal(eng.unet_forward(x, 500.0, [3]).cpu(), before)
    small = eng.unet_forward(x[..., :half, :half].contiguous(), 500.0, [2])      # slot 2 is not controlled: any size runs
    assert bool(torch.isfinite(small).all())
    with pytest.raises(RtError) as e:                                            # a hint larger than the plan
        eng.set_control_hint(torch.zeros(3, 16 * c["hw"], 8 * c["hw"], device=DEV))
    assert e.value.code == -1
    with pytest.raises(RtError):                                                 # the binding's own shape check
        eng.set_control_hint(torch.zeros(4, 8 * c["hw"], 8 * c["hw"], device=DEV))
    assert torch.equal(eng.unet_forward(x, 500.0, [3]).cpu(), before)
    off = _engine(c["cfg"], c["hw"], c["hw"], c["sd"])
    try:
        _rich_setup(off, c, control=False)
        want = off.unet_forward(x, 500.0, [3]).cpu()
        for call in (lambda: off.set_control_hint(c["hint"].to(DEV)), lambda: off.set_control_scales([1.0] * 4), lambda: off.set_control_hint(None),
                     lambda: off.control_embedding()):
            with pytest.raises(RtError) as e:
                call()
            assert e.value.code == -1
            assert torch.equal(off.unet_forward(x, 500.0, [3]).cpu(), want)
    finally:
        off.close()


# ---------------------------------------------------------------------------------------------------------------- facade
def _facade(which, c, cn=None):
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    m = RegionDiffusionXL(device=0, unet_state_dict=c["sd"], config=c["cfg"]) if which == "xl" else RegionDiffusion(0, unet_state_dict=c["sd"], config=c["cfg"])
    m.masks = [c["masks"][r:r + 1] for r in range(c["masks"].shape[0])]
    if cn is not None:
        m.load_controlnet(cn)
    return m


def test_facade_xl_window_changes_exactly_the_steps_inside_it():
    """tiny XL, 5 steps, set_control(start=0.2, end=0.6): steps 1 and 2 are controlled.  The rich pass (latents after every step, through
    the callback): step 0 equals the uncontrolled run bit for bit, step 1 differs; the whole run equals a hand-driven engine loop that
    switches the scales on before step 1 and off before step 3; the plain pass honours the window too; clear_control() and
    unload_controlnet() restore the bits of a pipeline that never loaded one."""
    c = R.rich_case()
    hw, R_, n = c["hw"], c["masks"].shape[0], 5
    tfd = {"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])}
    hint_u8 = (c["hint"] * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()

    def sample(m, rich=True):
        steps = []
        out = m.sample(prompt=None, height=8 * hw, width=8 * hw, num_inference_steps=n, guidance_scale=c["gs"], latents=c["lat"].clone() / c["sched"].init_noise_sigma,
                       prompt_embeds=c["emb"][1:] if rich else c["emb"][-1:], negative_prompt_embeds=c["emb"][:1],
                       pooled_prompt_embeds=c["pooled"][1:] if rich else c["pooled"][-1:], negative_pooled_prompt_embeds=c["pooled"][:1], output_type="latent",
                       run_rich_text=rich, text_format_dict=tfd, inject_selfattn=c["isa"], inject_background=c["ibg"],
                       callback=lambda i, t, lat: steps.append(lat.clone().cpu())).images.cpu()
        return out, steps
    never, never_steps = sample(_facade("xl", c))
    never_plain, _ = sample(_facade("xl", c), rich=False)
    m = _facade("xl", c, c["cn"])
    assert torch.equal(sample(m)[0], never)                                      # a ControlNet without a control request: off is off
    m.set_control(image=hint_u8, scale=0.8, regions={1: 0.0}, negative=0.7, start=0.2, end=0.6)
    on, on_steps = sample(m)
    assert len(on_steps) == n
    assert torch.equal(on_steps[0], never_steps[0]) and not torch.equal(on_steps[1], never_steps[1])
    assert rel_l2(on, never) > 1e-2 and torch.equal(sample(m)[0], on)
    on_plain, _ = sample(m, rich=False)
    assert rel_l2(on_plain, never_plain) > 1e-2
    # by hand
    eng = _engine(c["cfg"], hw, hw, c["sd_cn"], controlnet=CN)
    try:
        eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
        eng.set_control_hint(c["hint"].to(DEV))
        eng.set_masks(c["masks"].to(DEV))
        eng.set_fontsize(tfd["word_pos"], tfd["font_size"])
        m.scheduler.set_timesteps(n)
        eng.set_schedule(m.scheduler.kind, m.scheduler.timesteps.tolist(), m.scheduler.table(), n)
        eng.set_latents((c["lat"].clone() / c["sched"].init_noise_sigma).to(DEV).float() * m.scheduler.init_noise_sigma)
        scales = [0.7, 0.8, 0.0, 0.8]                                            # [negative, region 0, region 1, base]
        for i in range(n):
            if i == 1:
                eng.set_control_scales(scales)
            if i == 3:
                eng.set_control_scales([0.0] * 4)
            eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=True)
            assert torch.equal(eng.read_latents(hw, hw).cpu(), on_steps[i]), i
    finally:
        eng.close()
    with pytest.raises(ValueError):                                              # region 2 of a request with two region prompts
        m.set_control(image=hint_u8, regions={2: 0.5})
        sample(m)
    m.clear_control()
    assert torch.equal(sample(m)[0], never)
    m.unload_controlnet()
    assert torch.equal(sample(m)[0], never) and m.controlnet is None


def test_facade_sd_both_passes_honour_the_window():
    """tiny SD (PNDM), produce_latents and plain_latents with set_control(start=0.2, end=0.6) differ from the run without, repeat bit for
    bit, equal a hand-driven engine loop, and clear_control() restores the bits of a pipeline that never loaded a ControlNet."""
    from oracle.unet import TINY_SD_CONFIG, random_state_dict
    from rich_text_to_image_amd.controlnet import control_window
    from rich_text_to_image_amd.schedulers import PNDMTables
    cfg = TINY_SD_CONFIG
    g = torch.Generator().manual_seed(31)
    hw, R_, n = 32, 3, 5
    c = dict(cfg=cfg, sd=random_state_dict(cfg, seed=12), masks=torch.softmax(torch.randn(R_, 1, hw, hw, generator=g) * 2, 0).repeat(1, 4, 1, 1))
    emb = torch.randn(R_ + 1, 77, cfg["cross_attention_dim"], generator=g)
    lat = torch.randn(1, 4, hw, hw, generator=g)
    cn = R.control_state_dict(cfg, seed=23)
    hint = R.make_hint(hw, hw, seed=7)

    def rich(m):
        return m.produce_latents(emb, height=8 * hw, width=8 * hw, num_inference_steps=n, guidance_scale=7.5, latents=lat.clone(),
                                 inject_selfattn=0.5, inject_background=0.4).cpu()

    def plain(m):
        return m.plain_latents(emb[[0, R_]], 8 * hw, 8 * hw, n, 7.5, lat.clone()).cpu()
    m0 = _facade("sd", c)
    never_r, never_p = rich(m0), plain(m0)
    m = _facade("sd", c, cn)
    m.set_control(image=hint, scale=0.9, regions={0: 0.4}, start=0.2, end=0.6)          # a float [3, H, W] hint is taken as is
    on_r, on_p = rich(m), plain(m)
    assert rel_l2(on_r, never_r) > 1e-2 and rel_l2(on_p, never_p) > 1e-2
    assert torch.equal(rich(m), on_r) and torch.equal(plain(m), on_p)
    t = PNDMTables().set_timesteps(n)
    window = set(control_window(len(t.timesteps), 0.2, 0.6))
    assert 0 < len(window) < len(t.timesteps)
    eng = _engine(cfg, hw, hw, {**c["sd"], **R.prefixed(cn)}, controlnet=CN)
    try:
        def hand(emb_, scales, is_rich):
            eng.set_prompts(emb_.to(DEV))
            eng.set_control_hint(hint.to(DEV))
            eng.set_fontsize(None, None)
            eng.set_schedule(1, t.timesteps.tolist(), t.table(), n)
            eng.set_latents(lat.to(DEV))
            if is_rich:
                eng.set_masks(c["masks"].to(DEV))
            for i in range(len(t.timesteps)):
                if i in window and (i - 1) not in window:
                    eng.set_control_scales(scales)
                if i not in window and (i - 1) in window:
                    eng.set_control_scales([0.0] * len(scales))
                if is_rich:
                    eng.region_step(i, 7.5, 0.5, 0.4, xl=False)
                else:
                    eng.plain_step(i, 7.5)
            return eng.read_latents(hw, hw).cpu()
        assert torch.equal(on_r, hand(emb, [0.9, 0.4, 0.9, 0.9], True))
        assert torch.equal(on_p, hand(emb[[0, R_]], [0.9, 0.9], False))
        assert not torch.equal(on_r, hand(emb, [0.9, 0.9, 0.9, 0.9], True))          # what the comparison would catch: a dropped region scale
    finally:
        eng.close()
    m.clear_control()
    assert torch.equal(rich(m), never_r) and torch.equal(plain(m), never_p)
