"""FreeU on the GPU (csrc/freeu.hip, rt_set_freeu / rt_op_freeu): the op against the fp64 restatement of tests/freeu_ref.py at the bar
whose allowance tests/test_freeu.py measures, batch invariance, the memory contract, the forward against FreeUOracleUNet with all stream
modes, off-is-off, the refusal, the split step, graph capture and the facade."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import freeu_ref as R  # noqa: E402
from freeu_ref import FORWARD_BAR, FORWARD_FREEU, forward_case, oracle_streams, rel_l2  # noqa: E402
from memguard import damage, guarded, intact  # noqa: E402
from oracle.schedulers import OracleEuler  # noqa: E402
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict  # noqa: E402

DEV = "cuda:0"
FU = (FORWARD_FREEU["s1"], FORWARD_FREEU["s2"], FORWARD_FREEU["b1"], FORWARD_FREEU["b2"])


def _freeu(hidden, skip, H, W, b=1.0, s=1.0):
    from rich_text_to_image_amd.engine import freeu
    return freeu(hidden, skip, H, W, b, s)


# ---------------------------------------------------------------------------------------------------------------- the op
OP_CASES = [(g, c, B) for g in R.OP_GRIDS for c in (R.OP_CHANNELS_LARGE if g in R.LARGE_GRIDS else R.OP_CHANNELS_SMALL) for B in R.OP_STREAMS]


@pytest.mark.parametrize("grid,chan,B", OP_CASES, ids=[f"{g[0]}x{g[1]}-C{c[0]}+{c[1]}-B{B}" for g, c, B in OP_CASES])
def test_op_matches_the_fp64_restatement(grid, chan, B):
    """Skip half: every element within 2^-11 |ref| + 2^-25 + A |s - 1| max|sk| of the fp64 restatement, s in {0.2, 0.9, 1.5}.  Backbone
    half: bit-exact against (x.float() * b).half() on channels < C1 // 2, untouched bits above."""
    (H, W), (C1, C2) = grid, chan
    hid0, sk0 = (t[:B, :, :C].contiguous().to(DEV) for t, C in zip(R.op_inputs(H, W), (C1, C2)))
    maps = R.to_maps(sk0, H, W)
    for s, b in zip(R.OP_S, (1.4, 0.7, 2.0)):
        hid, sk = _freeu(hid0.clone(), sk0.clone(), H, W, b, s)
        ref = R.skip_ref(maps, s)
        ratio = ((R.to_maps(sk, H, W).double() - ref).abs() / R.bar(ref, maps, s)).max().item()
        print(f"freeu op {H}x{W} C1 {C1} C2 {C2} B {B} s {s}: worst |got - ref| / bar = {ratio:.3f}")
        assert ratio <= 1.0
        half = C1 // 2
        assert torch.equal(hid[..., :half], (hid0[..., :half].float() * b).half())
        assert torch.equal(hid[..., half:], hid0[..., half:])
        ratio_b = ((hid.double() - R.backbone_ref(hid0, b)).abs() / R.round_bar(R.backbone_ref(hid0, b))).max().item()
        assert ratio_b <= 1.0


@pytest.mark.parametrize("grid,chan", [((3, 5), (64, 32)), ((8, 12), (64, 32)), ((32, 32), (640, 320))])
def test_op_is_batch_invariant_and_deterministic(grid, chan):
    """Stream k of a launch of seven equals the same stream launched alone, bit for bit, and a second run equals the first."""
    (H, W), (C1, C2) = grid, chan
    hid0, sk0 = (t[:, :, :C].contiguous().to(DEV) for t, C in zip(R.op_inputs(H, W), (C1, C2)))
    hid, sk = _freeu(hid0.clone(), sk0.clone(), H, W, 1.4, 0.2)
    hid2, sk2 = _freeu(hid0.clone(), sk0.clone(), H, W, 1.4, 0.2)
    assert torch.equal(hid, hid2) and torch.equal(sk, sk2)
    assert not torch.equal(sk, sk0) and not torch.equal(hid, hid0)
    for k in (0, 3, 6):
        h1, s1 = _freeu(hid0[k:k + 1].clone(), sk0[k:k + 1].clone(), H, W, 1.4, 0.2)
        assert torch.equal(h1[0], hid[k]) and torch.equal(s1[0], sk[k]), k


@pytest.mark.parametrize("grid,chan,B", [((3, 5), (40, 24), 3), ((8, 12), (72, 40), 2), ((32, 32), (136, 72), 2)])
def test_op_memory_contract(grid, chan, B):
    """Both tensors inside guarded windows (tests/memguard.py), channel counts that are no multiple of the 32-channel slab (and C1 // 2
    no multiple of the 8-channel vector): the guards stay intact, every interior element is finite and meets the bar, and the half that
    is switched off (s == 1, b == 1) keeps its bytes."""
    (H, W), (C1, C2) = grid, chan
    g = torch.Generator().manual_seed(H * 31 + W)
    hid0 = (torch.randn(B, H * W, C1, generator=g) + 2.0 * torch.randn(C1, generator=g)).half().to(DEV)
    sk0 = (torch.randn(B, H * W, C2, generator=g) + 2.0 * torch.randn(C2, generator=g)).half().to(DEV)

    def windows():
        bh, vh = guarded((B * H * W, C1), torch.float16, device=DEV)
        bs, vs = guarded((B * H * W, C2), torch.float16, device=DEV)
        vh.copy_(hid0.reshape(-1, C1)); vs.copy_(sk0.reshape(-1, C2))
        assert vh.is_contiguous() and vs.is_contiguous()
        return bh, vh.view(B, H * W, C1), vh, bs, vs.view(B, H * W, C2), vs
    for b, s in ((1.4, 0.2), (1.0, 0.2), (1.4, 1.0), (1.0, 1.0)):
        bh, hid, vh, bs, sk, vs = windows()
        _freeu(hid, sk, H, W, b, s)
        assert intact(bh, vh), damage(bh, vh)
        assert intact(bs, vs), damage(bs, vs)
        assert bool(torch.isfinite(hid.float()).all()) and bool(torch.isfinite(sk.float()).all())
        if b == 1.0:
            assert torch.equal(hid.view(torch.int16), hid0.view(torch.int16))
        else:
            assert torch.equal(hid[..., :C1 // 2], (hid0[..., :C1 // 2].float() * b).half()) and torch.equal(hid[..., C1 // 2:], hid0[..., C1 // 2:])
        if s == 1.0:
            assert torch.equal(sk.view(torch.int16), sk0.view(torch.int16))
        else:
            maps = R.to_maps(sk0, H, W)
            ref = R.skip_ref(maps, s)
            assert ((R.to_maps(sk, H, W).double() - ref).abs() / R.bar(ref, maps, s)).max().item() <= 1.0
    # a NULL pointer skips its half
    bh, hid, vh, bs, sk, vs = windows()
    _freeu(None, sk, H, W, 1.4, 0.2)
    _freeu(hid, None, H, W, 1.4, 0.2)
    assert intact(bh, vh) and intact(bs, vs) and not torch.equal(sk, sk0) and not torch.equal(hid, hid0)


def test_op_refuses_what_it_cannot_do():
    from rich_text_to_image_amd.engine import RtError
    x = torch.randn(1, 4, 16).half().to(DEV)
    for H, W in ((1, 4), (4, 1)):
        with pytest.raises(RtError) as e:
            _freeu(None, x.clone(), H, W, 1.0, 0.5)
        assert e.value.code == -5
    y = x.clone()
    _freeu(y, None, 1, 4, 1.5, 1.0)                     # the backbone half has no such limit
    assert torch.equal(y[..., :8], (x[..., :8].float() * 1.5).half())
    for b, s in ((0.0, 0.5), (1.5, -1.0), (float("nan"), 0.5), (1.5, float("inf"))):
        with pytest.raises(RtError):
            _freeu(x.clone().reshape(1, 4, 16), x.clone().reshape(1, 4, 16), 2, 2, b, s)
    with pytest.raises(RtError):                        # channel counts are multiples of 8
        _freeu(None, torch.randn(1, 4, 12).half().to(DEV), 2, 2, 1.0, 0.5)


# ---------------------------------------------------------------------------------------------------------------- the forward
def _engine(cfg, h, w, sd, **kw):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(cfg, h, w, device=0, **kw)
    e.load_state_dict(sd)
    assert e.weights_missing()[0] == 0
    return e


def _engine_streams(eng, c):
    if c["xl"]:
        eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
    else:
        eng.set_prompts(c["emb"].to(DEV))
    eng.set_fontsize(c["wp"], c["fs"])
    x = torch.cat([c["lat"], c["lat"], c["lat_ref"], c["lat"]]).to(DEV)
    return eng.unet_forward(x, c["t"], [0, 2, 2, 1], fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2]).cpu()


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_forward_with_stream_modes_matches_the_freeu_oracle(which):
    """set_freeu, then one batched forward of uncond / base + font size / text_ref / injected region: every stream within the project's
    forward bar of FreeUOracleUNet - and more than ten bars away from the engine's own forward without FreeU.  Off is off: the forward
    before set_freeu, after disable_freeu() and after set_freeu(1, 1, 1, 1) give equal bits."""
    c = forward_case(which)
    eng = _engine(c["cfg"], c["h"], c["w"], c["sd"])
    try:
        before = _engine_streams(eng, c)
        eng.set_freeu(*FU)
        on = _engine_streams(eng, c)
        ref = oracle_streams(R.FreeUOracleUNet(c["cfg"], c["sd"], **FORWARD_FREEU), c)
        for k, name in enumerate(("uncond", "base+fontsize", "text_ref", "region injected")):
            r, d = rel_l2(on[k], ref[k]), rel_l2(on[k], before[k])
            print(f"{which} stream {name}: rel-L2 vs FreeU oracle {r:.3e}; vs the engine's FreeU-off forward {d:.3e}")
            assert r < FORWARD_BAR, name
            assert d > 10 * FORWARD_BAR, name
        alone = eng.unet_forward(c["lat"].to(DEV), c["t"], [0]).cpu()          # batch invariance survives FreeU, bit for bit
        assert torch.equal(alone[0], on[0])
        eng.disable_freeu()
        assert torch.equal(_engine_streams(eng, c), before)
        eng.set_freeu(*FU)
        eng.set_freeu(1, 1, 1, 1)
        assert torch.equal(_engine_streams(eng, c), before)
        plain = oracle_streams(OracleUNet(c["cfg"], c["sd"]), c)
        assert rel_l2(before[0], plain[0]) < FORWARD_BAR
    finally:
        eng.close()


def test_set_freeu_checks_its_arguments():
    from rich_text_to_image_amd.engine import RtError
    c = forward_case("xl")
    eng = _engine(c["cfg"], c["h"], c["w"], c["sd"])
    try:
        eng.set_freeu(*FU)
        on = _engine_streams(eng, c)
        for bad in ((0.0, 1, 1, 1), (1, -0.5, 1, 1), (1, 1, float("nan"), 1), (1, 1, 1, float("inf"))):
            with pytest.raises(RtError) as e:
                eng.set_freeu(*bad)
            assert e.value.code == -1
        assert torch.equal(_engine_streams(eng, c), on)                       # a refused call leaves the setting alone
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- steps
def _rich_case(hw=32, R_=3, steps=3, seed=77):
    cfg = TINY_XL_CONFIG
    g = torch.Generator().manual_seed(seed)
    sched = OracleEuler(); sched.set_timesteps(steps)
    return dict(cfg=cfg, sd=random_state_dict(cfg, seed=12), hw=hw, steps=steps, sched=sched,
                emb=torch.randn(R_ + 1, 77, cfg["cross_attention_dim"], generator=g), pooled=torch.randn(R_ + 1, 32, generator=g),
                tid=torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]]),
                masks=torch.softmax(torch.randn(R_, 1, hw, hw, generator=g) * 2, 0).repeat(1, 4, 1, 1),
                lat=torch.randn(1, 4, hw, hw, generator=g) * sched.init_noise_sigma, gs=5.0, isa=0.5, ibg=0.4)


def _rich_setup(eng, c):
    eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
    eng.set_masks(c["masks"].to(DEV))
    eng.set_fontsize(torch.tensor([3, 5]), torch.tensor([4.0, -2.0]))


def _rich_reset(eng, c):
    eng.set_schedule(0, c["sched"].timesteps.tolist(), c["sched"].sigmas.tolist(), c["steps"])
    eng.set_latents(c["lat"].to(DEV))


def _rich_loop(eng, c):
    _rich_reset(eng, c)
    for i in range(c["steps"]):
        eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=True)
    return eng.read_latents(c["hw"], c["hw"], with_ref=True)


@pytest.fixture(scope="module")
def rich():
    c = _rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd"])
    _rich_setup(eng, c)
    yield c, eng
    eng.close()


def test_off_is_off_in_the_region_loop(rich):
    """A 3-step region loop with FreeU switched on and off again equals the loop of an engine that never heard of FreeU, bit for bit; with
    FreeU on it does not."""
    c, eng = rich
    fresh = _engine(c["cfg"], c["hw"], c["hw"], c["sd"])
    try:
        _rich_setup(fresh, c)
        want = _rich_loop(fresh, c)
    finally:
        fresh.close()
    eng.set_freeu(*FU)
    on = _rich_loop(eng, c)
    eng.disable_freeu()
    off = _rich_loop(eng, c)
    assert torch.equal(off[0], want[0]) and torch.equal(off[1], want[1])
    assert rel_l2(on[0].cpu(), want[0].cpu()) > 1e-2


def test_split_step_equals_the_whole_step_with_freeu(rich):
    """rt_region_step_part for both parts of two, then _finish, equals rt_region_step with FreeU on: every stream gets the operator and
    its result is a function of that stream alone."""
    c, eng = rich
    eng.set_freeu(*FU)
    try:
        for i in (0, c["steps"] - 1):                      # an injected step (7 streams) and one without injection
            _rich_reset(eng, c)
            eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=True)
            whole = eng.read_latents(c["hw"], c["hw"], with_ref=True)
            _rich_reset(eng, c)
            ranges = [eng.region_step_part(i, c["gs"], c["isa"], c["ibg"], True, part, 2)[:2] for part in (0, 1)]
            assert all(n > 0 for _, n in ranges), ranges
            eng.region_step_finish(i, c["gs"], c["isa"], c["ibg"], True)
            parts = eng.read_latents(c["hw"], c["hw"], with_ref=True)
            assert torch.equal(parts[0], whole[0]) and torch.equal(parts[1], whole[1]), i
    finally:
        eng.disable_freeu()


def test_region_step_with_freeu_is_hipgraph_capturable(rich):
    """As test_region_step_is_hipgraph_capturable (tests/test_engine_gpu.py), with FreeU on: nothing is allocated and nothing
    synchronises inside the step, and the replay gives the eager step's bits."""
    c, eng = rich
    hw = c["hw"]
    eng.set_freeu(*FU)
    _rich_reset(eng, c)
    eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
    eager = eng.read_latents(hw, hw).clone()
    side = torch.cuda.Stream()
    eng.synchronize()
    eng.set_stream(side.cuda_stream)
    try:
        _rich_reset(eng, c)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
        for _ in range(2):
            _rich_reset(eng, c)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(eng.read_latents(hw, hw), eager)
    finally:
        torch.cuda.synchronize()
        eng.set_stream(None)
        eng.disable_freeu()
    _rich_reset(eng, c)


def test_a_1x1_stage_is_refused_before_anything_runs():
    """Tiny SD at 8 x 8 latents: the deepest grid is 1 x 1, where the filter's bins {-1, 0} do not exist.  With FreeU enabled the
    forward and the step raise RT_E_UNSUPPORTED naming FreeU, and the latents keep their bits."""
    from rich_text_to_image_amd.engine import RtError
    from oracle.schedulers import OraclePNDM
    cfg = TINY_SD_CONFIG
    eng = _engine(cfg, 32, 32, random_state_dict(cfg, seed=11))
    try:
        g = torch.Generator().manual_seed(3)
        eng.set_prompts(torch.randn(2, 77, cfg["cross_attention_dim"], generator=g).to(DEV))
        sched = OraclePNDM(); sched.set_timesteps(3)
        eng.set_schedule(1, sched.timesteps.tolist(), sched.alphas_cumprod.tolist(), 3)
        lat = torch.randn(1, 4, 8, 8, generator=g).to(DEV)
        eng.set_latents(lat)
        eng.set_freeu(*FU)
        for call in (lambda: eng.plain_step(0, 7.5), lambda: eng.unet_forward(lat, 500.0, [0])):
            with pytest.raises(RtError) as e:
                call()
            assert e.value.code == -5 and "FreeU" in str(e.value)
        assert torch.equal(eng.read_latents(8, 8), lat)
    finally:
        eng.close()


# ---------------------------------------------------------------------------------------------------------------- the facade
def test_facade_enable_freeu_changes_the_sample_and_disable_restores_it():
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    c = _rich_case()
    m = RegionDiffusionXL(device=0, unet_state_dict=c["sd"], config=c["cfg"])
    R_ = c["masks"].shape[0]
    m.masks = [c["masks"][r:r + 1] for r in range(R_)]
    hw = c["hw"]

    def sample():
        return m.sample(prompt=None, height=8 * hw, width=8 * hw, num_inference_steps=3, guidance_scale=c["gs"], latents=c["lat"].clone() / c["sched"].init_noise_sigma,
                        prompt_embeds=c["emb"][1:], negative_prompt_embeds=c["emb"][:1], pooled_prompt_embeds=c["pooled"][1:],
                        negative_pooled_prompt_embeds=c["pooled"][:1], output_type="latent", run_rich_text=True,
                        text_format_dict={"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])},
                        inject_selfattn=c["isa"], inject_background=c["ibg"]).images.cpu()
    base = sample()
    m.enable_freeu(*FU)
    on = sample()
    assert rel_l2(on, base) > 1e-2
    assert torch.equal(sample(), on)
    m.disable_freeu()
    assert torch.equal(sample(), base)
