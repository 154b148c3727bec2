"""The rich-text loops through the two facades on latent grids with h != w (tiny trace configs, live fp32 oracle):

  RegionDiffusion.produce_latents           PLMS             latent 64x96          vs oracle.region_loop.rich_loop_sd
  RegionDiffusionXL.sample(run_rich_text)   Euler            latent 80x48, 48x80   vs oracle.region_loop.rich_loop_xl

Each loop crosses the injection boundary and the background blend, is called with height = 8 h, width = 8 w and the facade's
default time_ids; the oracle's time_ids are built here, independently, as original_size + crops + target_size with (height, width).
Plus one colour-guided case per pipeline (VaeDecoder built at h x w, the precise one for XL, image-size colour masks that are not
square), one DPM-Solver++ case and one image-start case with pinned pixels (keep_source) against tests/img2img_ref.py.

On a square grid a swapped (h, w) - in a stride, the stride-2 down-sampler, the up-sampler phase pack, rt_set_masks / rt_set_source,
the VAE, the colour masks, the time_ids - computes the right answer.  Here it does not: every plain loop test carries its own
NEGATIVE CONTROL, the oracle evaluated on the transposed problem and transposed back, which must lie at least 10 x the test's bar
away from the oracle's answer (it is a statement about the test's discriminating power, not about the engine).

Bars (tests/test_engine_gpu.py): loops rel-L2 <= 3e-2 on the final latents at CFG 5.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import region_loop  # noqa: E402
from oracle.schedulers import OracleEuler, OraclePNDM  # noqa: E402
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict  # noqa: E402
from tests.dpm_solver_ref import RefDPMSolver  # noqa: E402
from tests.img2img_ref import ref_schedule, source_blend_ref  # noqa: E402

BAR, GS = 3e-2, 5.0


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


def _case(cfg, h, w, R, seed, xl):
    g = torch.Generator().manual_seed(seed)
    c = {"emb": torch.randn(R + 1, 77, cfg["cross_attention_dim"], generator=g), "pooled": torch.randn(R + 1, 32, generator=g) if xl else None,
         "lat": torch.randn(1, 4, h, w, generator=g)}
    m = torch.softmax(torch.randn(R, 1, h, w, generator=g) * 2, 0).repeat(1, 4, 1, 1)          # random: not symmetric under transposition
    c["masks"] = [m[r:r + 1] for r in range(R)]
    c["tfd"] = {"word_pos": torch.tensor([2, 3]), "font_size": torch.tensor([2.0, -1.5])}
    original_size = target_size = (8.0 * h, 8.0 * w)                                           # (height, width), xl.py:539-553
    c["tid"] = torch.tensor([list(original_size + (0.0, 0.0) + target_size)]) if xl else None
    return c


def _sd_model(sd, **kw):
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    return RegionDiffusion(0, unet_state_dict=sd, config=TINY_SD_CONFIG, **kw)


def _xl_model(sd, **kw):
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    return RegionDiffusionXL(device=0, unet_state_dict=sd, config=TINY_XL_CONFIG, **kw)


def _xl_sample(m, c, h, w, steps, **kw):
    """height / width only: original_size, target_size and so the time_ids are the facade's defaults."""
    kw.setdefault("latents", c["lat"].clone())
    if kw["latents"] is None:
        del kw["latents"]
    return m.sample(prompt=None, height=8 * h, width=8 * w, num_inference_steps=steps, guidance_scale=GS, prompt_embeds=c["emb"][1:],
                    negative_prompt_embeds=c["emb"][:1], pooled_prompt_embeds=c["pooled"][1:], negative_pooled_prompt_embeds=c["pooled"][:1],
                    output_type="latent", run_rich_text=True, text_format_dict=c["tfd"], **kw).images.cpu()


def _T(x):
    return x.transpose(-1, -2).contiguous()


def _crosses(timesteps, isa, ibg):
    """The schedule has injected and non-injected iterations, and the blend iteration lies inside it."""
    inj = [float(t) > (1 - isa) * 1000 for t in timesteps]
    assert any(inj) and not all(inj), inj
    assert 0 < int(ibg * len(timesteps)) < len(timesteps)


# ------------------------------------------------------------------------------------------------ plain rich loops + negative control
def test_region_diffusion_plms_loop_at_64x96_matches_oracle_loop():
    h, w, R, steps, isa, ibg = 64, 96, 2, 6, 0.5, 0.3              # 7 PLMS iterations; the 6144-token level of the live oracle is the clock (~100 s)
    sd = random_state_dict(TINY_SD_CONFIG, seed=13)
    c = _case(TINY_SD_CONFIG, h, w, R, 101, False)
    o = OracleUNet(TINY_SD_CONFIG, sd)
    s = OraclePNDM(); s.set_timesteps(steps)
    _crosses(s.timesteps, isa, ibg)
    ref = region_loop.rich_loop_sd(o, OraclePNDM(), c["emb"], c["masks"], c["lat"], steps, GS, c["tfd"], isa, ibg)
    m = _sd_model(sd)
    m.masks = c["masks"]
    kw = dict(height=8 * h, width=8 * w, num_inference_steps=steps, guidance_scale=GS, text_format_dict=c["tfd"], inject_selfattn=isa, inject_background=ibg)
    out = m.produce_latents(c["emb"], latents=c["lat"].clone(), **kw).cpu()
    assert tuple(out.shape) == (1, 4, h, w)
    r = rel_l2(out, ref)
    print(f"RegionDiffusion.produce_latents (PLMS, {len(s.timesteps)} iterations) @{h}x{w} vs oracle loop: rel-L2 {r:.3e}")
    assert r < BAR
    elided = m.produce_latents(c["emb"], latents=c["lat"].clone(), elide_dead_forwards=True, **kw).cpu()
    assert torch.equal(elided, out) or rel_l2(elided, out) < 1e-6
    # without latents the facade draws them at (height // 8, width // 8)
    assert tuple(m.produce_latents(c["emb"], **dict(kw, num_inference_steps=1)).shape) == (1, 4, h, w)
    # negative control: the transposed problem, transposed back
    swapped = _T(region_loop.rich_loop_sd(o, OraclePNDM(), c["emb"], [_T(x) for x in c["masks"]], _T(c["lat"]), steps, GS, c["tfd"], isa, ibg))
    d = rel_l2(swapped, ref)
    print(f"  negative control (oracle on the transposed problem, transposed back): rel-L2 {d:.3e}")
    assert d > 10 * BAR


@pytest.mark.parametrize("h,w", [(80, 48), (48, 80)], ids=["portrait_80x48", "landscape_48x80"])
def test_region_diffusion_xl_euler_loop_matches_oracle_loop(h, w):
    R, steps, isa, ibg = 2, 6, 0.5, 0.3
    sd = random_state_dict(TINY_XL_CONFIG, seed=14)
    c = _case(TINY_XL_CONFIG, h, w, R, 102, True)
    o = OracleUNet(TINY_XL_CONFIG, sd)
    s = OracleEuler(); s.set_timesteps(steps)
    _crosses(s.timesteps, isa, ibg)
    lat0 = c["lat"] * s.init_noise_sigma
    ref = region_loop.rich_loop_xl(o, OracleEuler(), c["emb"], c["pooled"], c["tid"], c["masks"], lat0, steps, GS, c["tfd"], isa, ibg)
    m = _xl_model(sd)
    m.masks = c["masks"]
    out = _xl_sample(m, c, h, w, steps, inject_selfattn=isa, inject_background=ibg)
    assert tuple(out.shape) == (1, 4, h, w)
    r = rel_l2(out, ref)
    print(f"RegionDiffusionXL.sample (Euler, {steps} steps) @{h}x{w} vs oracle loop: rel-L2 {r:.3e}")
    assert r < BAR
    elided = _xl_sample(m, c, h, w, steps, inject_selfattn=isa, inject_background=ibg, elide_dead_forwards=True)
    assert torch.equal(elided, out) or rel_l2(elided, out) < 1e-6
    assert tuple(_xl_sample(m, c, h, w, 1, latents=None).shape) == (1, 4, h, w)
    # negative controls: the transposed problem (latents, masks, and height <-> width in the time_ids), transposed back; and height <-> width
    # in the time_ids alone
    tid_swapped = c["tid"][:, [1, 0, 3, 2, 5, 4]]
    swapped = _T(region_loop.rich_loop_xl(o, OracleEuler(), c["emb"], c["pooled"], tid_swapped, [_T(x) for x in c["masks"]], _T(lat0), steps, GS,
                                          c["tfd"], isa, ibg))
    d = rel_l2(swapped, ref)
    ids_only = region_loop.rich_loop_xl(o, OracleEuler(), c["emb"], c["pooled"], tid_swapped, c["masks"], lat0, steps, GS, c["tfd"], isa, ibg)
    print(f"  negative control (oracle on the transposed problem, transposed back): rel-L2 {d:.3e}; time_ids (width, height) alone: {rel_l2(ids_only, ref):.3e}")
    assert d > 10 * BAR
    assert rel_l2(ids_only, ref) > BAR                            # (width, height) in the time_ids alone cannot pass either


# ------------------------------------------------------------------------------------------------ colour guidance
def _guidance_inputs(h, w, g, tfd):
    cm = [torch.rand(1, 1, 8 * h, 8 * w, generator=g).repeat(1, 4, 1, 1) for _ in range(2)]                # image-size masks, not square
    return dict(tfd, target_RGB=[torch.rand(1, 3, 1, 1, generator=g) for _ in range(2)], guidance_start_step=999, color_guidance_weight=0.5,
                color_obj_atten=cm, color_obj_atten_all=torch.rand(1, 4, h, w, generator=g))


@pytest.mark.parametrize("xl,h,w", [(False, 64, 96), (True, 80, 48)], ids=["sd_64x96", "xl_80x48"])
def test_colour_guided_loop_off_the_square_matches_oracle_loop(xl, h, w):
    """tests/test_facade_gpu.py::test_colour_guided_loop_matches_oracle_loop with h != w: region loop + colour guidance through a
    VaeDecoder built at h x w (XL: the precise one, as the reference decodes in fp32 there) + background blend."""
    from oracle.vae import TINY_VAE_CONFIG, OracleVAEDecoder, random_vae_state_dict
    from rich_text_to_image_amd.engine import VaeDecoder
    cfg = TINY_XL_CONFIG if xl else TINY_SD_CONFIG
    R, steps, isa, ibg = 2, 3, 0.5, 0.5
    sd = random_state_dict(cfg, seed=15)
    vsd = random_vae_state_dict(TINY_VAE_CONFIG, seed=2)
    c = _case(cfg, h, w, R, 103, xl)
    tfd = _guidance_inputs(h, w, torch.Generator().manual_seed(7), c["tfd"])
    guidance = {"vae": OracleVAEDecoder(TINY_VAE_CONFIG, vsd), "scaling": TINY_VAE_CONFIG["scaling_factor"]}
    vae = VaeDecoder(TINY_VAE_CONFIG, h, w, device=0, state_dict=vsd, precise=xl)
    o = OracleUNet(cfg, sd)
    c = dict(c, tfd=tfd)
    if xl:
        s = OracleEuler(); s.set_timesteps(steps)
        ref = region_loop.rich_loop_xl(o, OracleEuler(), c["emb"], c["pooled"], c["tid"], c["masks"], c["lat"] * s.init_noise_sigma, steps, GS, tfd, isa, ibg,
                                       use_guidance=True, guidance=guidance)
        m = _xl_model(sd, vae=vae, vae_scaling_factor=TINY_VAE_CONFIG["scaling_factor"])
        m.masks = c["masks"]
        out = _xl_sample(m, c, h, w, steps, use_guidance=True, inject_selfattn=isa, inject_background=ibg)
        plain = _xl_sample(m, c, h, w, steps, use_guidance=False, inject_selfattn=isa, inject_background=ibg)
    else:
        ref = region_loop.rich_loop_sd(o, OraclePNDM(), c["emb"], c["masks"], c["lat"], steps, GS, tfd, isa, ibg, use_guidance=True, guidance=guidance)
        m = _sd_model(sd, vae=vae)
        m.masks = c["masks"]
        kw = dict(height=8 * h, width=8 * w, num_inference_steps=steps, guidance_scale=GS, text_format_dict=tfd, inject_selfattn=isa, inject_background=ibg)
        out = m.produce_latents(c["emb"], latents=c["lat"].clone(), use_guidance=True, **kw).cpu()
        plain = m.produce_latents(c["emb"], latents=c["lat"].clone(), use_guidance=False, **kw).cpu()
    vae.close()
    r, moved = rel_l2(out, ref), rel_l2(plain, out)
    print(f"colour-guided rich loop ({'xl' if xl else 'sd'}) @{h}x{w} vs oracle loop: rel-L2 {r:.3e}; guidance moved the result by {moved:.3e}")
    assert moved > 1e-4                                          # the guidance step really ran
    assert r < BAR


# ------------------------------------------------------------------------------------------------ DPM-Solver++
def test_region_diffusion_xl_dpm_loop_at_48x80_matches_oracle_loop():
    from rich_text_to_image_amd.schedulers import DPMSolverTables
    h, w, R, steps, isa, ibg = 48, 80, 2, 8, 0.5, 0.3
    sd = random_state_dict(TINY_XL_CONFIG, seed=16)
    c = _case(TINY_XL_CONFIG, h, w, R, 104, True)
    m = _xl_model(sd)
    m.scheduler = DPMSolverTables()
    m.masks = c["masks"]
    out = _xl_sample(m, c, h, w, steps, inject_selfattn=isa, inject_background=ibg)
    _crosses(m.scheduler.timesteps, isa, ibg)
    ref = region_loop.rich_loop_xl(OracleUNet(TINY_XL_CONFIG, sd), RefDPMSolver(), c["emb"], c["pooled"], c["tid"], c["masks"], c["lat"], steps, GS,
                                   c["tfd"], isa, ibg)
    r = rel_l2(out, ref)
    print(f"RegionDiffusionXL DPM-Solver++ @{h}x{w} vs oracle loop: rel-L2 {r:.3e}")
    assert r < BAR


# ------------------------------------------------------------------------------------------------ image start with pinned pixels
class _PinnedEuler(OracleEuler):
    """The oracle's Euler scheduler on the truncated tables of tests/img2img_ref.py, with what rt_source_blend does after every
    iteration restated in fp64 (img2img_ref.source_blend_ref) on the latent stream (row 0; the reference stream is not pinned)."""

    def __init__(self, r, x0, noise, keep):
        super().__init__()
        self._r, self._pin, self._i = r, (x0, noise, keep), 0

    def set_timesteps(self, n, device=None):
        super().set_timesteps(n)
        self.timesteps = torch.from_numpy(self._r["timesteps"].copy())
        self.sigmas = torch.from_numpy(self._r["sigmas"].copy())
        self._i = 0

    def step(self, eps, t, sample):
        prev = super().step(eps, t, sample)["prev_sample"].clone()
        a, b = self._r["levels"][self._i]
        self._i += 1
        prev[:1] = source_blend_ref(prev[:1], *self._pin, a, b).float()
        return {"prev_sample": prev}


def test_image_start_with_pinned_rows_at_80x48_matches_pinned_oracle_loop():
    """strength 0.5 of 8 Euler steps from a source latent, self-attention injection on, the top rows pinned to the source
    (keep_source; a band of ROWS: its transpose is a band of columns).  inject_background = 0, so that the pin directly follows the
    scheduler step and _PinnedEuler restates the loop exactly."""
    h, w, R, n, strength, isa = 80, 48, 2, 8, 0.5, 0.8
    sd = random_state_dict(TINY_XL_CONFIG, seed=17)
    c = _case(TINY_XL_CONFIG, h, w, R, 105, True)
    g = torch.Generator().manual_seed(53)
    x0, noise = 0.8 * torch.randn(1, 4, h, w, generator=g), torch.randn(1, 4, h, w, generator=g)
    keep = torch.zeros(h, w)
    keep[:h // 4] = 1.0
    keep[h // 4:h // 4 + 8] = torch.rand(8, w, generator=g)                   # a soft edge
    r = ref_schedule("euler", n, strength)
    assert any(float(t) > (1 - isa) * 1000 for t in r["timesteps"])
    a, b = r["start"]
    start = (a * x0.double() + b * noise.double()).float()
    ref = region_loop.rich_loop_xl(OracleUNet(TINY_XL_CONFIG, sd), _PinnedEuler(r, x0, noise, keep), c["emb"], c["pooled"], c["tid"], c["masks"], start, n,
                                   GS, c["tfd"], isa, 0.0)
    free = region_loop.rich_loop_xl(OracleUNet(TINY_XL_CONFIG, sd), _PinnedEuler(r, x0, noise, torch.zeros(h, w)), c["emb"], c["pooled"], c["tid"], c["masks"],
                                    start, n, GS, c["tfd"], isa, 0.0)
    m = _xl_model(sd)
    m.masks = c["masks"]
    out = _xl_sample(m, c, h, w, n, latents=None, image=x0.cuda(), strength=strength, noise=noise.cuda(), keep_source=keep.cuda(), inject_selfattn=isa,
                     inject_background=0.0)
    assert len(m.scheduler.timesteps) == len(r["timesteps"])
    e = rel_l2(out, ref)
    print(f"image start, rows pinned @{h}x{w} vs pinned oracle loop: rel-L2 {e:.3e}; the pin moved the oracle's result by {rel_l2(free, ref):.3e}")
    assert e < BAR
    assert torch.equal(out[..., :h // 4, :], x0[..., :h // 4, :])            # the last level is (1, 0): the source's bits
    assert rel_l2(free, ref) > 10 * BAR                                      # the pin matters: a misplaced keep mask would show


# ------------------------------------------------------------------------------------------------ engine capacity vs stepped size
def _modes_and_step(eng, c, h, w):
    """The stream-mode forward of tests/test_engine_gpu.py and one injected rich step (Euler) at h x w -> (forward, latents, reference latents)."""
    R = len(c["masks"])
    eng.set_prompts(c["emb"].cuda(), c["pooled"].cuda(), c["tid"])
    eng.set_fontsize(c["tfd"]["word_pos"], c["tfd"]["font_size"])
    g = torch.Generator().manual_seed(9)
    x = torch.randn(4, 4, h, w, generator=g).cuda()
    fwd = eng.unet_forward(x, 701.0, [0, 2, 2, 1], fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2])
    plain = eng.unet_forward(x, 701.0, [0, 2, 2, 1])
    assert rel_l2(plain[1], fwd[1]) > 1e-3 and rel_l2(plain[3], fwd[3]) > 1e-3          # the mode words matter
    s = OracleEuler(); s.set_timesteps(2)
    eng.set_masks(torch.cat(c["masks"]).cuda())
    eng.set_schedule(0, s.timesteps.tolist(), s.sigmas.tolist(), 2)
    eng.set_latents((c["lat"] * s.init_noise_sigma).cuda())
    eng.region_step(0, GS, 0.5, 0.0, xl=True, elide=False)
    lat, ref = eng.read_latents(h, w, with_ref=True)
    assert R == 2 and rel_l2(lat, c["lat"] * s.init_noise_sigma) > 1e-3
    return fwd, lat, ref


@pytest.mark.parametrize("h,w", [(32, 48), (48, 80)], ids=["halved_32x48", "not_a_halving_48x80"])
def test_engine_built_at_64x96_steps_smaller_grids_like_an_engine_of_that_size(h, w):
    """The C ABI lets an engine built at (H, W) be stepped at any admissible smaller (h, w); rt_create dry-runs the halved sizes only,
    and the split-K scratch grows as maps shrink.  Workspace::alloc refuses an overflow on the host before anything is launched and
    launch_split takes its own (re-allocated) buffer when the engine's is too small, so a smaller grid either runs or raises - and
    when it runs, every route is a function of the problem shape, not of the capacity: the bits of an engine built at exactly h x w."""
    from rich_text_to_image_amd.engine import Engine
    sd = random_state_dict(TINY_XL_CONFIG, seed=18)
    c = _case(TINY_XL_CONFIG, h, w, 2, 106, True)
    outs = []
    for H, W in ((64, 96), (h, w)):
        eng = Engine(TINY_XL_CONFIG, H, W, device=0)
        eng.load_state_dict(sd)
        outs.append(_modes_and_step(eng, c, h, w))
        eng.close()
    for name, a, b in zip(("stream-mode forward", "latents after a rich step", "reference latents after a rich step"), *outs):
        assert torch.equal(a, b), f"{name} at {h}x{w}: an engine built at 64x96 and one built at {h}x{w} differ by rel-L2 {rel_l2(a, b):.3e}"
    # and the answer is the oracle's (the forward; the loops above cover the step)
    o = OracleUNet(TINY_XL_CONFIG, sd)
    x0 = torch.randn(4, 4, h, w, generator=torch.Generator().manual_seed(9))[:1]
    with torch.no_grad():
        ref = o.forward(x0, 701.0, c["emb"][:1], {"text_embeds": c["pooled"][:1], "time_ids": c["tid"]})
    r = rel_l2(outs[0][0][0], ref[0])
    print(f"engine built at 64x96, forward at {h}x{w}: uncond stream vs oracle rel-L2 {r:.3e}")
    assert r < 1.5e-2


# ------------------------------------------------------------------------------------------------ sizes that are refused
def test_a_grid_whose_attention_level_is_not_a_multiple_of_8_tokens_is_refused():
    """SDXL's 1216x832 bucket: latent 152x104, whose 38x26 level has 988 tokens.  Attention levels need h*w % 8 == 0 (DESIGN.md
    section 8): the engine says so at construction (or, for an engine built larger, at the forward) - no result, no fault."""
    from rich_text_to_image_amd.engine import Engine, RtError
    for h, w in ((152, 104), (104, 152)):
        with pytest.raises(RtError) as err:
            eng = Engine(TINY_XL_CONFIG, h, w, device=0)
            eng.load_state_dict(random_state_dict(TINY_XL_CONFIG, seed=18))
            c = _case(TINY_XL_CONFIG, h, w, 2, 107, True)
            eng.set_prompts(c["emb"].cuda(), c["pooled"].cuda(), c["tid"])
            eng.unet_forward(c["lat"].cuda(), 701.0, [0])
        assert "multiple of 8" in str(err.value), str(err.value)
    # an engine with room for it refuses the forward
    eng = Engine(TINY_XL_CONFIG, 160, 160, device=0)
    eng.load_state_dict(random_state_dict(TINY_XL_CONFIG, seed=18))
    c = _case(TINY_XL_CONFIG, 152, 104, 2, 107, True)
    eng.set_prompts(c["emb"].cuda(), c["pooled"].cuda(), c["tid"])
    with pytest.raises(RtError) as err:
        eng.unet_forward(c["lat"].cuda(), 701.0, [0])
    assert "multiple of 8" in str(err.value), str(err.value)
    ok = _case(TINY_XL_CONFIG, 144, 112, 2, 107, True)                    # 1152x896: 36x28 = 1008 tokens, runs (on the same engine, after the refusal)
    out = eng.unet_forward(ok["lat"].cuda(), 701.0, [0])
    assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
    eng.close()
