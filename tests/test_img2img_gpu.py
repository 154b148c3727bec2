"""Image start on the GPU: rt_set_source / rt_noise_latents / rt_source_blend (csrc/step.hip) against the fp64 restatement
(tests/img2img_ref.py), the truncated loops of the engine with and without pinned pixels, the truncated rich loops of both facades
against the in-repo CPU oracle, the facades' new keyword arguments, and graph capture of a step followed by the pin."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import region_loop  # noqa: E402
from oracle.schedulers import OracleEuler, OraclePNDM  # noqa: E402
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict  # noqa: E402
from tests.img2img_ref import blend_bound, noise_latents_ref, ref_schedule, source_blend_ref  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


def _gold(name):
    return torch.load(os.path.join(GOLD, name + ".pt"))


def make_engine(cfg, hw, sd):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(cfg, hw, hw, device=0)
    e.load_state_dict(sd)
    assert e.weights_missing()[0] == 0
    return e


@pytest.fixture(scope="module")
def tiny_xl():
    sd = random_state_dict(TINY_XL_CONFIG, seed=11)
    return TINY_XL_CONFIG, sd, make_engine(TINY_XL_CONFIG, 128, sd)


@pytest.fixture(scope="module")
def tiny_sd():
    sd = random_state_dict(TINY_SD_CONFIG, seed=11)
    return TINY_SD_CONFIG, sd, make_engine(TINY_SD_CONFIG, 64, sd)


def _tables(kind, n, strength):
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerTables, PNDMTables
    return {"euler": EulerTables, "pndm": PNDMTables, "dpm": DPMSolverTables}[kind]().set_timesteps(n, strength)


def _bind(eng, xl):
    """Prompts, masks and font sizes of the golden case on the engine -> (golden, latent size)."""
    g = _gold("tiny_xl_euler" if xl else "tiny_sd_plms")
    inp = g["inputs"]
    if xl:
        eng.set_prompts(inp["embeds"].to(DEV), inp["pooled"].to(DEV), inp["time_ids"])
    else:
        eng.set_prompts(inp["embeds"].to(DEV))
    eng.set_masks(inp["masks"].repeat(1, 4, 1, 1).to(DEV))
    eng.set_fontsize(inp["word_pos"], inp["font_size"])
    return g, inp["latents"].shape[2]


def _source(hw, seed):
    g = torch.Generator().manual_seed(seed)
    return (0.8 * torch.randn(1, 4, hw, hw, generator=g)).to(DEV), torch.randn(1, 4, hw, hw, generator=g).to(DEV)


def _schedule(eng, t, n):
    eng.set_schedule(t.kind, t.timesteps.tolist(), t.table(), n)


def _within_bound(got, want64, bound64, what):
    err = (got.double().cpu() - want64.cpu()).abs()
    worst = (err / bound64.cpu().clamp_min(1e-300)).max().item()
    print(f"{what}: max |err| {err.max().item():.3e}, worst err / bound {worst:.3f}")
    assert bool((err <= bound64.cpu()).all()), (what, worst)


# ------------------------------------------------------------------------------------------------ 3: the two kernels
def test_noise_latents_and_source_blend_match_the_fp64_restatement():
    """|err| <= 4 * 2^-24 * (|a x0| + |b noise| + |lat|) per element (img2img_ref.blend_bound), keep = 0, 1 and fractional,
    levels including (1, 0); the exact cases; the state errors."""
    from rich_text_to_image_amd.engine import Engine, RtError
    hw = 32
    e = Engine(TINY_SD_CONFIG, hw, hw, device=0)
    g = torch.Generator().manual_seed(31)
    x0 = (0.8 * torch.randn(1, 4, hw, hw, generator=g)).to(DEV)
    noise = torch.randn(1, 4, hw, hw, generator=g).to(DEV)
    lat0 = (3.0 * torch.randn(1, 4, hw, hw, generator=g)).to(DEV)
    keep = torch.rand(hw, hw, generator=g)
    keep[:8] = 0.0
    keep[8:16] = 1.0
    keep = keep.to(DEV)
    with pytest.raises(RtError) as err:
        e.noise_latents(1.0, 1.0)
    assert err.value.code == -3
    with pytest.raises(RtError) as err:
        e.source_blend(1.0, 1.0)
    assert err.value.code == -3
    e.set_source(x0, noise, keep)
    zero = torch.zeros_like(x0)
    for a, b in ((1.0, 0.0), (1.0, 14.614642), (1.0, 0.0413), (0.0683, 0.99766), (0.7071, 0.7071), (0.99957, 0.02915)):
        e.noise_latents(a, b)
        lat, ref = e.read_latents(hw, hw, with_ref=True)
        assert torch.equal(lat, ref)
        _within_bound(lat, noise_latents_ref(x0, noise, a, b), blend_bound(zero, x0, noise, a, b), f"noise_latents({a}, {b})")
        e.set_latents(lat0)
        e.source_blend(a, b)
        lat, ref = e.read_latents(hw, hw, with_ref=True)
        _within_bound(lat, source_blend_ref(lat0, x0, noise, keep, a, b), blend_bound(lat0, x0, noise, a, b), f"source_blend({a}, {b})")
        assert torch.equal(ref, lat0)                                   # the reference stream is not touched
        assert torch.equal(lat[..., :8, :], lat0[..., :8, :])           # keep == 0 leaves the bits alone
        if (a, b) == (1.0, 0.0):
            assert torch.equal(lat[..., 8:16, :], x0[..., 8:16, :])     # keep == 1 at the level (1, 0): the source's bits
    e.set_source(x0, noise, None)                                       # no keep mask: a no-op
    e.set_latents(lat0)
    e.source_blend(0.5, 0.5)
    assert torch.equal(e.read_latents(hw, hw), lat0)
    e.set_source(None)
    with pytest.raises(RtError) as err:
        e.source_blend(1.0, 0.0)
    assert err.value.code == -3
    e.set_source(x0[..., :16, :16].contiguous(), noise[..., :16, :16].contiguous(), keep[:16, :16].contiguous())
    e.set_latents(lat0)
    with pytest.raises(RtError):                                        # source and latents differ in shape
        e.source_blend(1.0, 0.0)
    e.close()


# ------------------------------------------------------------------------------------------------ 4: strength 1, bit-identical
def _rich_loop(eng, t, g, xl, isa=0.5, ibg=0.3, levels=None, trace=None, hw=None):
    for i in range(len(t.timesteps)):
        eng.region_step(i, g["guidance_scale"], isa, ibg, xl=xl)
        if levels is not None:
            eng.source_blend(*levels[i])
        if trace is not None:
            trace.append(eng.read_latents(hw, hw))


@pytest.mark.parametrize("kind", ["euler", "pndm", "dpm"])
def test_strength_one_image_start_is_bit_identical_to_set_latents(kind, tiny_xl, tiny_sd):
    xl = kind == "euler"
    cfg, sd, eng = tiny_xl if xl else tiny_sd
    g, hw = _bind(eng, xl)
    n = 6
    t = _tables(kind, n, 1.0)
    x0, noise = _source(hw, 41)
    _schedule(eng, t, n)
    eng.set_source(x0, noise)
    eng.noise_latents(*t.start_level())
    start, start_ref = eng.read_latents(hw, hw, with_ref=True)
    assert torch.equal(start, start_ref)
    _rich_loop(eng, t, g, xl)
    a, a_ref = eng.read_latents(hw, hw, with_ref=True)
    eng.set_source(None)
    _schedule(eng, t, n)
    eng.set_latents(start)                                   # what rt_noise_latents itself produced
    _rich_loop(eng, t, g, xl)
    b, b_ref = eng.read_latents(hw, hw, with_ref=True)
    assert torch.equal(a, b) and torch.equal(a_ref, b_ref)
    assert rel_l2(a, start) > 1e-2                            # the loop ran


# ------------------------------------------------------------------------------------------------ 5, 6: pinned pixels
def _pinned_run(eng, g, xl, kind, n, strength, hw, keep, x0, noise):
    t = _tables(kind, n, strength)
    _schedule(eng, t, n)
    eng.set_source(x0, noise, keep)
    eng.noise_latents(*t.start_level())
    trace = []
    _rich_loop(eng, t, g, xl, levels=t.source_levels(), trace=trace, hw=hw)
    eng.set_source(None)
    return t, trace


@pytest.mark.parametrize("strength", [0.3, 0.8])
@pytest.mark.parametrize("kind", ["euler", "pndm", "dpm"])
def test_keep_everything_returns_the_source(kind, strength, tiny_xl, tiny_sd):
    xl = kind == "euler"
    cfg, sd, eng = tiny_xl if xl else tiny_sd
    g, hw = _bind(eng, xl)
    x0, noise = _source(hw, 43)
    t, trace = _pinned_run(eng, g, xl, kind, 10, strength, hw, torch.ones(hw, hw, device=DEV), x0, noise)
    assert len(trace) == len(t.timesteps)
    for i, ((a, b), lat) in enumerate(zip(t.source_levels(), trace)):
        want = noise_latents_ref(x0, noise, a, b)
        _within_bound(lat, want, blend_bound(want, x0, noise, a, b), f"{kind} strength {strength} iteration {i}")
    assert torch.equal(trace[-1], x0)


@pytest.mark.parametrize("kind", ["euler", "pndm"])
def test_half_plane_keep_pins_its_half_and_steers_the_other(kind, tiny_xl, tiny_sd):
    xl = kind == "euler"
    cfg, sd, eng = tiny_xl if xl else tiny_sd
    g, hw = _bind(eng, xl)
    x0, noise = _source(hw, 47)
    keep = torch.zeros(hw, hw, device=DEV)
    keep[:, :hw // 2] = 1.0
    t, kept = _pinned_run(eng, g, xl, kind, 10, 0.8, hw, keep, x0, noise)
    _, free = _pinned_run(eng, g, xl, kind, 10, 0.8, hw, None, x0, noise)          # source_blend without a keep mask: a no-op
    L, Rt = (Ellipsis, slice(0, hw // 2)), (Ellipsis, slice(hw // 2, hw))
    for i, ((a, b), lat) in enumerate(zip(t.source_levels(), kept)):
        want = noise_latents_ref(x0, noise, a, b)
        _within_bound(lat[L], want[L], blend_bound(want, x0, noise, a, b)[L], f"{kind} kept half, iteration {i}")
        if i == 0:
            assert torch.equal(lat[Rt], free[0][Rt])         # the first step saw the same latents
        else:
            r = rel_l2(lat[Rt], free[i][Rt])                 # later steps see the pinned neighbours
            print(f"{kind} free half, iteration {i}: rel-L2 to the unpinned run {r:.3e}")
            assert r > 1e-4, (i, r)
    assert torch.equal(kept[-1][L], x0[L])


# ------------------------------------------------------------------------------------------------ facades
def _sd_model(seed, **kw):
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    return RegionDiffusion(0, unet_state_dict=random_state_dict(TINY_SD_CONFIG, seed=seed), config=TINY_SD_CONFIG, **kw)


def _xl_model(seed, **kw):
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    return RegionDiffusionXL(device=0, unet_state_dict=random_state_dict(TINY_XL_CONFIG, seed=seed), config=TINY_XL_CONFIG, **kw)


def _encoder(lat_hw, precise):
    from rich_text_to_image_amd.engine import VaeEncoder
    from oracle.vae import TINY_VAE_CONFIG
    from tests.vae_encoder_ref import random_vae_encoder_state_dict
    return VaeEncoder(TINY_VAE_CONFIG, lat_hw, lat_hw, device=0, state_dict=random_vae_encoder_state_dict(TINY_VAE_CONFIG, seed=6), precise=precise)


@pytest.fixture(scope="module")
def xl_case():
    from oracle.vae import TINY_VAE_CONFIG
    g = _gold("tiny_xl_euler")
    m = _xl_model(g["weight_seed"], vae_encoder=_encoder(128, True), vae_scaling_factor=TINY_VAE_CONFIG["scaling_factor"])
    m.masks = [x[None].repeat(1, 4, 1, 1) for x in g["inputs"]["masks"]]
    return g, m


@pytest.fixture(scope="module")
def sd_case():
    g = _gold("tiny_sd_plms")
    m = _sd_model(g["weight_seed"], vae_encoder=_encoder(64, False))
    m.masks = [x[None].repeat(1, 4, 1, 1) for x in g["inputs"]["masks"]]
    return g, m


def _xl_sample(m, g, steps, **kw):
    inp = g["inputs"]
    hw = inp["latents"].shape[2] * 8
    kw.setdefault("run_rich_text", True)
    if kw["run_rich_text"]:
        kw.setdefault("text_format_dict", {"word_pos": inp["word_pos"], "font_size": inp["font_size"]})
    emb, pooled = (inp["embeds"], inp["pooled"]) if kw["run_rich_text"] else (inp["embeds"][[0, -1]], inp["pooled"][[0, -1]])
    return m.sample(prompt=None, height=hw, width=hw, num_inference_steps=steps, guidance_scale=g["guidance_scale"],
                    prompt_embeds=emb[1:], negative_prompt_embeds=emb[:1], pooled_prompt_embeds=pooled[1:],
                    negative_pooled_prompt_embeds=pooled[:1], output_type="latent", original_size=(hw, hw), target_size=(hw, hw),
                    **kw).images


def _sd_latents(m, g, steps, **kw):
    inp = g["inputs"]
    kw.setdefault("text_format_dict", {"word_pos": inp["word_pos"], "font_size": inp["font_size"]})
    return m.produce_latents(inp["embeds"], num_inference_steps=steps, guidance_scale=g["guidance_scale"], **kw)


class _TruncEuler(OracleEuler):
    """The oracle's Euler scheduler with its tables overwritten after set_timesteps (the oracle loops call set_timesteps themselves)."""

    def __init__(self, r):
        super().__init__()
        self._r = r

    def set_timesteps(self, n, device=None):
        super().set_timesteps(n)
        self.timesteps = torch.from_numpy(self._r["timesteps"].copy())
        self.sigmas = torch.from_numpy(self._r["sigmas"].copy())


class _TruncPNDM(OraclePNDM):
    def __init__(self, r):
        super().__init__()
        self._r = r

    def set_timesteps(self, n, device=None):
        super().set_timesteps(n)                              # resets the counter and the history; the step ratio stays 1000 // n
        self.timesteps = torch.from_numpy(self._r["timesteps"].copy())


# ------------------------------------------------------------------------------------------------ 7: truncated rich loops vs the CPU oracle
@pytest.mark.parametrize("which", ["xl", "sd"])
def test_truncated_rich_loop_matches_oracle_loop(which, xl_case, sd_case):
    """strength 0.5 of 8 steps, self-attention injection above t = 200 and the background blend on, nothing pinned; the oracle loops
    of oracle/region_loop.py run the truncated tables of tests/img2img_ref.py.  rel-L2 < 3e-2, the figure of
    test_engine_gpu.py::test_rich_text_loop_matches_reference_golden for these loops."""
    xl = which == "xl"
    g, m = xl_case if xl else sd_case
    inp = g["inputs"]
    cfg = TINY_XL_CONFIG if xl else TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=g["weight_seed"])
    n, strength, isa, ibg = 8, 0.5, 0.8, 0.5
    hw = inp["latents"].shape[2]
    x0, noise = _source(hw, 53)
    r = ref_schedule("euler" if xl else "pndm", n, strength)
    assert any(float(t) > (1 - isa) * 1000 for t in r["timesteps"])          # the injection really runs
    a, b = r["start"]
    start = (a * x0.cpu().double() + b * noise.cpu().double()).float()
    tfd = {"word_pos": inp["word_pos"], "font_size": inp["font_size"]}
    if xl:
        tid = torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]])
        ref = region_loop.rich_loop_xl(OracleUNet(cfg, sd), _TruncEuler(r), inp["embeds"], inp["pooled"], tid, m.masks, start, n,
                                       g["guidance_scale"], tfd, isa, ibg)
        out = _xl_sample(m, g, n, image=x0, strength=strength, noise=noise, inject_selfattn=isa, inject_background=ibg)
    else:
        ref = region_loop.rich_loop_sd(OracleUNet(cfg, sd), _TruncPNDM(r), inp["embeds"], m.masks, start, n, g["guidance_scale"], tfd, isa, ibg)
        out = _sd_latents(m, g, n, image=x0, strength=strength, noise=noise, inject_selfattn=isa, inject_background=ibg)
    assert len(m.scheduler.timesteps) == len(r["timesteps"])
    e = rel_l2(out, ref)
    print(f"truncated rich loop ({which}, strength {strength}) vs oracle loop: rel-L2 {e:.3e}")
    assert e < 3e-2
    assert rel_l2(out, start) > 1e-2


# ------------------------------------------------------------------------------------------------ 8: the keyword arguments
@pytest.mark.parametrize("which", ["xl", "sd"])
def test_facade_image_arguments(which, xl_case, sd_case):
    xl = which == "xl"
    g, m = xl_case if xl else sd_case
    hw = g["inputs"]["latents"].shape[2]
    run = (lambda **kw: _xl_sample(m, g, 6, **kw)) if xl else (lambda **kw: _sd_latents(m, g, 6, **kw))
    gen = torch.Generator().manual_seed(59)
    pixels = torch.rand(1, 3, 8 * hw, 8 * hw, generator=gen)
    noise = torch.randn(1, 4, hw, hw, generator=gen)
    kw = dict(strength=0.7, noise=noise, inject_selfattn=0.5, inject_background=0.3)
    # pixels are encoded by encode_imgs; latents are taken as given
    torch.manual_seed(5)
    z = m.encode_imgs(pixels.to(DEV))
    assert z.shape == (1, 4, hw, hw)
    from_latents = run(image=z, **kw)
    torch.manual_seed(5)
    from_pixels = run(image=pixels, **kw)
    assert torch.equal(from_pixels, from_latents)
    assert torch.equal(run(image=z, **kw), from_latents)                        # fixed noise: deterministic
    assert rel_l2(run(image=z, **dict(kw, strength=0.4)), from_latents) > 1e-3  # the strength reaches the loop
    # default noise: drawn from the seeded RNG where `latents` is drawn
    torch.manual_seed(7)
    a = run(image=z, strength=0.7)
    torch.manual_seed(7)
    assert torch.equal(run(image=z, strength=0.7), a)
    # keep_source: everything kept returns the source's bits; "background" is the last region mask
    assert torch.equal(run(image=z, keep_source=torch.ones(hw, hw), **kw), z)
    bg = run(image=z, keep_source="background", **kw)
    assert torch.equal(bg, run(image=z, keep_source=m.masks[-1][:, :1], **kw))
    assert rel_l2(bg, from_latents) > 1e-3
    # errors
    lat = g["inputs"]["latents"].clone()
    with pytest.raises(ValueError):
        run(image=z, latents=lat, **kw)
    for bad in (0.0, 1.5, 0.05):                                                 # 0.05 of 6 steps: no solver step left
        with pytest.raises(ValueError):
            run(image=z, **dict(kw, strength=bad))
    with pytest.raises(ValueError):
        run(image=z, keep_source="foreground", **kw)
    m.split_image = True
    try:
        with pytest.raises(ValueError):
            run(image=z, keep_source="background", **kw)
    finally:
        m.split_image = False
    m.register_tokenmap_hooks()
    try:
        with pytest.raises(ValueError, match="10"):                              # 12 * 0.5 = 6 iterations: no maps would be recorded
            if xl:
                _xl_sample(m, g, 12, image=z, strength=0.5, noise=noise, run_rich_text=False)
            else:
                m.plain_latents(g["inputs"]["embeds"][[0, -1]], num_inference_steps=12, guidance_scale=7.5, image=z, strength=0.5, noise=noise)
    finally:
        m.remove_tokenmap_hooks()
    # image=None: nothing changes, down to the bits, and the other three arguments are not read
    today = run(latents=lat.clone(), inject_selfattn=0.5, inject_background=0.3)
    assert torch.equal(run(latents=lat.clone(), inject_selfattn=0.5, inject_background=0.3, image=None, strength=7.0,
                           noise=torch.ones(1), keep_source="background"), today)


def test_plain_pass_starts_from_the_image_too(xl_case, sd_case):
    """The plain (token-map) pass of both facades takes image / strength / noise, and with hooks and more than 10 iterations it records."""
    for (g, m), xl in ((xl_case, True), (sd_case, False)):
        hw = g["inputs"]["latents"].shape[2]
        x0, noise = _source(hw, 61)
        emb2 = g["inputs"]["embeds"][[0, -1]]

        def plain(**kw):
            if xl:
                return _xl_sample(m, g, 14, run_rich_text=False, **kw)
            return m.plain_latents(emb2, num_inference_steps=14, guidance_scale=g["guidance_scale"], **kw)
        a = plain(image=x0, strength=0.8, noise=noise)
        assert torch.equal(plain(image=x0, strength=0.8, noise=noise), a)
        assert rel_l2(plain(image=x0, strength=0.4, noise=noise), a) > 1e-3
        m.register_tokenmap_hooks()
        try:
            plain(image=x0, strength=0.8, noise=noise)           # 11 iterations
            recorded = list(m.selfattn_maps.values()) + list(m.crossattn_maps.values())
            assert any(torch.is_tensor(v) for v in recorded) and all(int(v) == 11 + (not xl) for v in m.n_maps.values())
        finally:
            m.remove_tokenmap_hooks()


# ------------------------------------------------------------------------------------------------ 9: graph capture
def test_region_step_with_source_blend_is_hipgraph_capturable(tiny_xl):
    """In the manner of test_engine_gpu.py::test_region_step_is_hipgraph_capturable: an injected rich-text step followed by
    rt_source_blend, captured on a side stream and replayed from the same start, gives the eager bits."""
    cfg, sd, eng = tiny_xl
    g, hw = _bind(eng, True)
    n = 6
    t = _tables("euler", n, 0.8)
    x0, noise = _source(hw, 67)
    keep = (torch.rand(hw, hw, generator=torch.Generator().manual_seed(3)) > 0.5).float().to(DEV)
    eng.set_source(x0, noise, keep)
    level = t.source_levels()[0]

    def reset():
        _schedule(eng, t, n)
        eng.noise_latents(*t.start_level())

    def step():
        eng.region_step(0, g["guidance_scale"], 0.8, 0.3, xl=True)
        eng.source_blend(*level)

    reset()
    step()
    eager = eng.read_latents(hw, hw).clone()
    reset()
    eng.region_step(0, g["guidance_scale"], 0.8, 0.3, xl=True)
    assert not torch.equal(eng.read_latents(hw, hw), eager)   # the pin is part of what is captured
    side = torch.cuda.Stream()
    eng.synchronize()
    eng.set_stream(side.cuda_stream)
    try:
        reset()
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            step()
        for _ in range(2):
            reset()
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(eng.read_latents(hw, hw), eager)
    finally:
        torch.cuda.synchronize()
        eng.set_stream(None)
        eng.set_source(None)


# ------------------------------------------------------------------------------------------------ the image driver
def test_generate_edits_an_image_and_keeps_its_background():
    """sample.generate with init_image / strength / keep_source="background" (what --init_image / --strength / --keep_source pass):
    both passes start from the once-encoded image, the token maps are recorded (13 executed iterations), and where the mask of the
    unformatted text is 1 the rich pass returns the latents of the image itself."""
    from rich_text_to_image_amd import img2img
    from rich_text_to_image_amd.sample import generate
    from tests.test_sample_gpu import _model
    js = {"ops": [{"insert": "a "}, {"attributes": {"font": "slabo"}, "insert": "night sky"}, {"insert": " above a "},
                  {"attributes": {"link": "a wooden fence covered in snow"}, "insert": "fence"}, {"insert": "\n"}]}
    param = {"text_input": js, "height": 512, "width": 512, "guidance_weight": 7.5, "steps": 14, "noise_index": 3, "negative_prompt": ""}
    m = _model()
    m.vae_encoder = _encoder(64, False)
    pixels = torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(71))
    seen = {}
    produce, source = m.produce_latents, img2img.source_latents

    def spy_produce(*a, **kw):
        seen["kw"], seen["out"] = kw, produce(*a, **kw)
        return seen["out"]

    def spy_source(model, image):
        out = source(model, image)
        if image.shape[1] == 3:
            seen["encodes"] = seen.get("encodes", 0) + 1
            seen["x0"] = out
        return out
    m.produce_latents = spy_produce
    img2img.source_latents = spy_source
    try:
        # segment_threshold 0.5: with these random weights the default 0.3 assigns every segment to a span (an empty background) and 0.6
        # none (nothing but background); 0.5 leaves both
        kw = dict(inject_selfattn=0.3, num_segments=5, inject_background=0.3, init_image=pixels, strength=0.9, segment_threshold=0.5)
        plain, rich, _ = generate(m, param, "SD", None, keep_source="background", **kw)
        kept_out, x0 = seen["out"], seen["x0"]
        assert seen["encodes"] == 1 and torch.equal(seen["kw"]["image"], x0) and seen["kw"]["keep_source"] == "background"
        assert plain.shape == (1, 512, 512, 3) and rich.shape == (1, 512, 512, 3)
        bg = (m.masks[-1][:, :1] == 1).expand(1, 4, 64, 64)
        free = (m.masks[-1][:, :1] < 0.5).expand(1, 4, 64, 64)
        print(f"background mask: {int(bg.sum()) // 4} pixels at 1, {int(free.sum()) // 4} below 0.5, of {64 * 64}")
        assert bg.any() and free.any()
        assert torch.equal(kept_out[bg], x0[bg])
        plain2, rich2, _ = generate(m, param, "SD", None, keep_source="background", **kw)
        assert (plain2 == plain).all() and (rich2 == rich).all() and torch.equal(seen["out"], kept_out)
        plain3, rich3, _ = generate(m, param, "SD", None, keep_source=None, **kw)
        assert (plain3 == plain).all()                                      # the plain pass does not pin
        assert not torch.equal(seen["out"][bg], x0[bg]) and rel_l2(seen["out"][free], kept_out[free]) > 1e-4
        with pytest.raises(ValueError, match="10"):                         # 14 * 0.5 = 7 solver steps: the hooks would record nothing
            generate(m, param, "SD", None, **dict(kw, strength=0.5))
    finally:
        img2img.source_latents = source


def test_sdxl_command_line_edits_an_image_from_a_checkpoint_directory(tmp_path):
    """`sample --model SDXL --init_image a.png --strength 0.9 --keep_source background` on a synthetic SDXL-layout checkpoint whose vae/
    holds encoder weights: RegionDiffusionXL.encode_imgs builds its (precise) VaeEncoder from vae/ on first use and matches the
    oracle encoder; the run writes both images, repeats to the byte, and differs from the run that starts from noise."""
    import json
    import numpy as np
    from PIL import Image
    from safetensors.torch import save_file
    from oracle.vae import TINY_VAE_CONFIG, random_vae_state_dict
    from rich_text_to_image_amd import sample
    from rich_text_to_image_amd.checkpoint import load_pipeline
    from tests.test_checkpoint_gpu import _write_xl_dir
    from tests.vae_encoder_ref import OracleVAEEncoder, random_vae_encoder_state_dict
    ckpt = str(tmp_path / "ckpt")
    _write_xl_dir(ckpt)
    vsd, esd = dict(random_vae_state_dict(TINY_VAE_CONFIG, seed=5)), random_vae_encoder_state_dict(TINY_VAE_CONFIG, seed=6)
    vsd.update(esd)
    save_file({k: v.contiguous() for k, v in vsd.items()}, os.path.join(ckpt, "vae", "diffusion_pytorch_model.safetensors"))
    m = load_pipeline(ckpt, "SDXL", device=0, latent_hw=(128, 128))
    pix = torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(73))
    torch.manual_seed(21)
    z = m.encode_imgs(pix)
    assert m._lazy_encoder[0].precise and z.shape == (1, 4, 32, 32)
    with torch.no_grad():
        mom = OracleVAEEncoder(TINY_VAE_CONFIG, esd).moments(2 * pix - 1)
    torch.manual_seed(21)
    eps = torch.randn(mom[:, :4].shape, device=DEV).cpu()
    want = (mom[:, :4] + torch.exp(0.5 * mom[:, 4:]) * eps) * m.vae_scaling_factor
    r = rel_l2(z, want)
    print(f"RegionDiffusionXL.encode_imgs (lazy precise encoder from vae/) vs oracle: rel-L2 {r:.3e}")
    assert r < 2e-2
    del m
    rgb = (torch.rand(300, 200, 3, generator=torch.Generator().manual_seed(75)) * 255).to(torch.uint8).numpy()
    Image.fromarray(rgb).save(tmp_path / "a.png")
    ja = json.dumps({"ops": [{"insert": "a "}, {"attributes": {"link": "a wooden fence covered in snow"}, "insert": "fence"}, {"insert": " and a "},
                             {"attributes": {"font": "slabo"}, "insert": "barn"}, {"insert": " under a night sky\n"}]})
    common = ["--load_path", ckpt, "--model", "SDXL", "--sample_steps", "14", "--num_segments", "4", "--inject_selfattn", "0.5",
              "--rich_text_json", ja, "--seed", "3"]
    edit = ["--init_image", str(tmp_path / "a.png"), "--strength", "0.9", "--keep_source", "background"]
    sample.main(common + edit + ["--run_dir", str(tmp_path / "out1")])
    sample.main(common + edit + ["--run_dir", str(tmp_path / "out2")])
    sample.main(common + ["--run_dir", str(tmp_path / "out0")])
    for kind in ("plain", "rich"):
        one = open(tmp_path / "out1" / f"seed3_{kind}.jpg", "rb").read()
        assert np.asarray(Image.open(tmp_path / "out1" / f"seed3_{kind}.jpg")).shape == (1024, 1024, 3)
        assert open(tmp_path / "out2" / f"seed3_{kind}.jpg", "rb").read() == one, kind
        assert open(tmp_path / "out0" / f"seed3_{kind}.jpg", "rb").read() != one, kind
