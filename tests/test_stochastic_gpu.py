"""The stochastic samplers on the GPU: the device noise field (csrc/philox.h) against the uint64 / fp64 restatement; the stochastic step
epilogues (csrc/step.hip step_epilogue_kernel<STEP_EULER_A / STEP_SDE> + step_driver.inl solver_coeffs / multistep_coeffs) against tests/sde_ref.py, without the UNet; seeds;
the field shared by the plain pass and the reference stream of the rich pass; both façades against the oracle loops driven by the
restated schedulers and fed the engine's own fields; the image start; the split-image command line."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import region_loop  # noqa: E402
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict  # noqa: E402
from tests.sde_ref import RefEulerAncestral, RefSdeDpmSolver, noise_field, noise_words  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
EULER_A, SDE_1, SDE_2 = 4, 5, 6


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


def _device_field(seed, h, w):
    """noise_fn of the restated schedulers: the engine's own field, read back (so the accuracy of the device normals does not enter)."""
    from rich_text_to_image_amd.engine import step_noise
    return lambda i: step_noise(seed, i, h, w).cpu()


# ------------------------------------------------------------------------------------------------ 1: the noise field
@pytest.mark.parametrize("seed,step,h,w", [(0, 0, 12, 8), (1234, 3, 25, 40), ((7 << 32) + 5, 49, 64, 65)],
                         ids=["96px_partial_block", "1000px", "4160px_high_key_word"])
def test_noise_field_on_the_device(seed, step, h, w):
    """Words bit for bit; normals within 2^-20 max(1, rad) of the fp64 restatement (about eight fp32 ulps: logf, sqrtf and sincospif
    at about two each)."""
    from rich_text_to_image_amd.engine import step_noise
    z, words = step_noise(seed, step, h, w, words=True)
    assert tuple(z.shape) == (1, 4, h, w) and tuple(words.shape) == (h * w, 4)
    assert np.array_equal(words.cpu().numpy().astype(np.uint64), noise_words(seed, step, h * w))
    z64, rad = noise_field(seed, step, h, w)
    err = np.abs(z[0].cpu().double().numpy() - z64)
    bar = 2.0 ** -20 * np.maximum(1.0, rad)
    print(f"device normals ({seed}, {step}, {h}x{w}): max |z - z64| {err.max():.3e}, worst err / bar {(err / bar).max():.3f}")
    assert (err <= bar).all(), (err / bar).max()
    assert torch.equal(step_noise(seed, step, h, w), z)                       # a pure function of its arguments


# ------------------------------------------------------------------------------------------------ 2: the epilogue alone
def _engine(eng_hw, n_prompts):
    """A tiny engine for the epilogue alone: the UNet never runs, so its arena is only marked bound."""
    from rich_text_to_image_amd.engine import Engine
    e = Engine(TINY_SD_CONFIG, eng_hw, eng_hw, device=0)
    e.arena_mark_bound()
    g = torch.Generator().manual_seed(9)
    e.set_prompts(torch.randn(n_prompts, 77, TINY_SD_CONFIG["cross_attention_dim"], generator=g).to(DEV))
    return e


def _eps_slots(e, h, w):
    from rich_text_to_image_amd.launcher import eps_tensor
    buf, per = eps_tensor(e)
    f = buf.view(torch.float32)
    n = per // 4
    assert n == 4 * h * w
    return lambda s, x: f[s * n:(s + 1) * n].copy_(x.reshape(4, h * w).t().reshape(-1))      # NCHW [1,4,h,w] -> the stream's NHWC slot


def _restated(kind, noise_fn, n):
    ref = RefEulerAncestral(noise_fn) if kind == EULER_A else RefSdeDpmSolver(noise_fn, 2 if kind == SDE_2 else 1)
    return ref.set_timesteps(n)


def _set_schedule(e, kind, ref, n):
    if kind == EULER_A:
        e.set_schedule(kind, ref.timesteps.tolist(), ref.sigmas.tolist(), n)
    else:
        e.set_schedule(kind, [float(t) for t in ref.timesteps.tolist()], ref.alphas_cumprod.tolist(), n)


def _epilogue_alone(mode, kind, h, w, eng_hw, seed=77, n=20, R=3, gs=7.5):
    isa, ibg = (0.5, 0.3) if mode == "sd" else (0.0, 0.3)
    xl = mode == "xl"
    e = _engine(eng_hw, 2 if mode == "plain" else R + 1)
    g = torch.Generator().manual_seed(4)
    masks = torch.softmax(torch.randn(R, 1, h, w, generator=g) * 2, 0).repeat(1, 4, 1, 1)
    if mode != "plain":
        e.set_masks([masks[r:r + 1].to(DEV) for r in range(R)])
    ref = _restated(kind, _device_field(seed, h, w), n)
    _set_schedule(e, kind, ref, n)
    e.set_noise_seed(seed)
    lat0 = torch.randn(1, 4, h, w, generator=g) * ref.init_noise_sigma
    e.set_latents(lat0.to(DEV))
    put = _eps_slots(e, h, w)
    lat, lat_ref = lat0.clone(), lat0.clone()
    M = [masks[r:r + 1] for r in range(R)]
    for i, t in enumerate(ref.timesteps.tolist()):
        if mode == "plain":
            eu, et = torch.randn(1, 4, h, w, generator=g), torch.randn(1, 4, h, w, generator=g)
            put(0, eu.to(DEV)); put(1, et.to(DEV))
            e.plain_step_finish(i, gs)
            lat = ref.step(eu + gs * (et - eu), t, lat)["prev_sample"]
        else:
            F = 4 + R - 1                                    # uncond, base, uncond_ref, text_ref, regions (no elision: the pair always runs)
            ep = [torch.randn(1, 4, h, w, generator=g) for _ in range(F)]
            for s in range(F):
                put(s, ep[s].to(DEV))
            e.region_step_finish(i, gs, isa, ibg, xl)
            nu, nt = ep[0] * M[-1], ep[1] * M[-1]
            for r in range(R - 1):
                nu = nu + ep[0] * M[r]
                nt = nt + ep[4 + r] * M[r]
            eps = nu + gs * (nt - nu)
            eps_ref = ep[2] + gs * (ep[3] - ep[2])
            step_ref = (isa > 0 or i < ibg * n) if xl else True
            if step_ref:
                out = ref.step(torch.cat([eps, eps_ref]), t, torch.cat([lat, lat_ref]))["prev_sample"]
                lat, lat_ref = out[:1], out[1:]
            else:
                lat = ref.step(eps, t, lat)["prev_sample"]
            if i == int(ibg * n):
                lat = lat_ref * M[-1] + lat * (1 - M[-1])
        got, got_ref = e.read_latents(h, w, with_ref=True)
        bar = 1e-5 * (i + 1) * lat.abs().max().item()
        err = (got.cpu() - lat).abs().max().item()
        assert err <= bar, (mode, kind, i, err, bar)
        if mode != "plain":
            err_ref = (got_ref.cpu() - lat_ref).abs().max().item()
            assert err_ref <= 1e-5 * (i + 1) * lat_ref.abs().max().item(), (mode, kind, i, "reference stream", err_ref)
    print(f"{mode} kind {kind} {h}x{w}: last-step L-inf {err:.3e} (bar {bar:.3e})")
    e.close()


@pytest.mark.parametrize("mode,kind", [("sd", SDE_1), ("sd", SDE_2), ("xl", SDE_1), ("xl", SDE_2), ("plain", SDE_1), ("plain", SDE_2),
                                       ("xl", EULER_A), ("plain", EULER_A)])
def test_epilogue_alone_matches_the_restatement(mode, kind):
    """Seeded noise predictions written straight into the eps buffer of every stream, then the step's finish: region mask combine + CFG
    + stochastic update of both streams with ONE field + blend, against the fp32 restatement fed the same CFG-combined predictions and
    the field read back from the device, every step."""
    _epilogue_alone(mode, kind, 32, 32, 32)


@pytest.mark.parametrize("mode,kind", [("sd", SDE_2), ("xl", EULER_A)])
def test_epilogue_alone_on_a_12x8_latent_of_a_32x32_engine(mode, kind):
    """96 pixels: the tail of the only block."""
    _epilogue_alone(mode, kind, 12, 8, 32)


def test_set_schedule_checks_the_tables_of_the_new_kinds():
    from rich_text_to_image_amd.engine import RtError
    e = _engine(32, 2)
    ref = _restated(EULER_A, None, 5)
    with pytest.raises(RtError):
        e.set_schedule(EULER_A, ref.timesteps.tolist(), ref.sigmas.tolist()[:-1], 5)            # Euler's tables: n + 1 sigmas
    with pytest.raises(RtError):
        e.set_schedule(SDE_2, [999.0, 500.0], ref.sigmas.tolist(), 2)                           # DPM's tables: alphas_cumprod[1000]
    with pytest.raises(RtError):
        e.set_schedule(7, [999.0], ref.alphas_cumprod.tolist(), 1)
    e.close()


# ------------------------------------------------------------------------------------------------ 3: seeds
def _plain_run(e, kind, seed, h=32, w=32, n=6):
    """A plain epilogue-only run with seeded predictions; seed None leaves the engine's noise seed alone."""
    from oracle.schedulers import OracleEuler, OraclePNDM
    g = torch.Generator().manual_seed(21)
    if kind in (EULER_A, SDE_1, SDE_2):
        ref = _restated(kind, None, n)
        _set_schedule(e, kind, ref, n)
        ts = ref.timesteps.tolist()
    elif kind == 0:
        o = OracleEuler(); o.set_timesteps(n)
        e.set_schedule(0, o.timesteps.tolist(), o.sigmas.tolist(), n)
        ts = o.timesteps.tolist()
    elif kind == 1:
        o = OraclePNDM(); o.set_timesteps(n)
        e.set_schedule(1, [float(t) for t in o.timesteps.tolist()], o.alphas_cumprod.tolist(), n)
        ts = o.timesteps.tolist()
    else:
        from tests.dpm_solver_ref import dpm_timesteps, scaled_linear_alphas_cumprod
        ts = dpm_timesteps(n).tolist()
        e.set_schedule(kind, [float(t) for t in ts], scaled_linear_alphas_cumprod().tolist(), n)
    if seed is not None:
        e.set_noise_seed(seed)
    e.set_latents(torch.randn(1, 4, h, w, generator=g).to(DEV))
    put = _eps_slots(e, h, w)
    for i in range(len(ts)):
        put(0, torch.randn(1, 4, h, w, generator=g).to(DEV)); put(1, torch.randn(1, 4, h, w, generator=g).to(DEV))
        e.plain_step_finish(i, 5.0)
    return e.read_latents(h, w).cpu()


def test_seeds():
    e = _engine(32, 2)
    for kind in (EULER_A, SDE_1, SDE_2):
        a = _plain_run(e, kind, 5)
        assert torch.equal(_plain_run(e, kind, 5), a), kind                       # the same seed twice
        assert torch.equal(_plain_run(e, kind, None), a), kind                    # the seed survives set_schedule and set_latents
        b = _plain_run(e, kind, 6)
        assert not torch.equal(a, b) and (a - b).abs().max().item() > 1e-2, kind
        assert not torch.equal(_plain_run(e, kind, 5 + (1 << 32)), a), kind       # the high word counts
    for kind in (1, 0, 3):                                                        # PNDM, Euler, DPM-Solver++ 2M ignore it
        assert torch.equal(_plain_run(e, kind, 0), _plain_run(e, kind, 123)), kind
    e.close()


def _sd_model(seed, **kw):
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    return RegionDiffusion(0, unet_state_dict=random_state_dict(TINY_SD_CONFIG, seed=seed), config=TINY_SD_CONFIG, **kw)


def _xl_model(seed, **kw):
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    return RegionDiffusionXL(device=0, unet_state_dict=random_state_dict(TINY_XL_CONFIG, seed=seed), config=TINY_XL_CONFIG, **kw)


def _xl_sample(m, inp, hw, steps, gs, **kw):
    return m.sample(prompt=None, height=hw, width=hw, num_inference_steps=steps, guidance_scale=gs, latents=inp["latents"].clone(),
                    prompt_embeds=inp["embeds"][1:], negative_prompt_embeds=inp["embeds"][:1], pooled_prompt_embeds=inp["pooled"][1:],
                    negative_pooled_prompt_embeds=inp["pooled"][:1], output_type="latent", original_size=(hw, hw), target_size=(hw, hw),
                    **kw).images


def test_default_schedulers_after_a_stochastic_run_are_untouched():
    """A stochastic run with a seed, then the default scheduler on the same object: the same latents as a fresh object."""
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables, EulerTables, PNDMTables
    g = torch.load(os.path.join(GOLD, "tiny_sd_plms.pt"))
    inp = g["inputs"]
    masks = [x[None].repeat(1, 4, 1, 1) for x in inp["masks"]]
    kw = dict(num_inference_steps=6, guidance_scale=7.5, text_format_dict={"word_pos": inp["word_pos"], "font_size": inp["font_size"]},
              inject_selfattn=0.5, inject_background=0.5)
    fresh = _sd_model(g["weight_seed"])
    fresh.masks = masks
    want = fresh.produce_latents(inp["embeds"], latents=inp["latents"].clone(), **kw)
    m = _sd_model(g["weight_seed"], scheduler=DPMSolverTables(algorithm="sde-dpmsolver++"))
    m.masks = masks
    sde = m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), noise_seed=9, **kw)
    assert rel_l2(sde, want) > 1e-3
    assert torch.equal(m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), noise_seed=9, **kw), sde)
    assert rel_l2(m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), noise_seed=10, **kw), sde) > 1e-3
    m.scheduler = PNDMTables()
    assert torch.equal(m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), **kw), want)
    with pytest.raises(ValueError):                        # SD-v1.5 has no sigma-space sampler
        m.scheduler = EulerAncestralTables()
        m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), **kw)

    gx = torch.load(os.path.join(GOLD, "tiny_xl_euler.pt"))
    ix = gx["inputs"]
    hw = ix["latents"].shape[2] * 8
    kx = dict(run_rich_text=True, text_format_dict={"word_pos": ix["word_pos"], "font_size": ix["font_size"]}, inject_selfattn=0.5, inject_background=0.5)
    mx = [x[None].repeat(1, 4, 1, 1) for x in ix["masks"]]
    fresh = _xl_model(gx["weight_seed"])
    fresh.masks = mx
    want = _xl_sample(fresh, ix, hw, 6, 5.0, **kx)
    m = _xl_model(gx["weight_seed"], scheduler=EulerAncestralTables())
    m.masks = mx
    assert rel_l2(_xl_sample(m, ix, hw, 6, 5.0, noise_seed=9, **kx), want) > 1e-3
    m.scheduler = EulerTables()
    assert torch.equal(_xl_sample(m, ix, hw, 6, 5.0, **kx), want)


# ------------------------------------------------------------------------------------------------ 4: one field for both passes
def _ref_stream_against_plain(eng, inp, tables, seed, n, gs=5.0, isa=0.5):
    """Per step: max |reference latents of the rich loop - latents of the plain loop| from the same start and seed, and whether the two
    are bit-identical."""
    hw = inp["latents"].shape[2]
    t = tables.set_timesteps(n)
    lat0 = (inp["latents"] * t.init_noise_sigma).to(DEV)
    eng.set_prompts(inp["embeds"][[0, -1]].to(DEV), inp["pooled"][[0, -1]].to(DEV), inp["time_ids"])
    eng.set_schedule(t.kind, t.timesteps.tolist(), t.table(), n)
    eng.set_noise_seed(seed)
    eng.set_latents(lat0)
    plain = []
    for i in range(n):
        eng.plain_step(i, gs)
        plain.append(eng.read_latents(hw, hw))
    eng.set_prompts(inp["embeds"].to(DEV), inp["pooled"].to(DEV), inp["time_ids"])
    eng.set_masks(inp["masks"].repeat(1, 4, 1, 1).to(DEV))
    eng.set_fontsize(inp["word_pos"], inp["font_size"])
    eng.set_schedule(t.kind, t.timesteps.tolist(), t.table(), n)
    eng.set_latents(lat0)
    diffs, same = [], []
    for i in range(n):
        eng.region_step(i, gs, isa, 0.0, xl=True)
        _, ref = eng.read_latents(hw, hw, with_ref=True)
        diffs.append((ref - plain[i]).abs().max().item())
        same.append(torch.equal(ref, plain[i]))
    assert (plain[-1] - lat0).abs().max().item() > 1e-2
    return diffs, same


def test_reference_stream_of_the_rich_pass_sees_the_noise_of_the_plain_pass():
    """Kind 4, inject_selfattn 0.5, 12 steps.  The same comparison with the deterministic Euler sampler sets the requirement: bit
    identity where Euler is bit-identical, else no further apart than twice Euler's distance at the same step."""
    from rich_text_to_image_amd.engine import Engine
    from rich_text_to_image_amd.schedulers import EulerAncestralTables, EulerTables
    g = torch.load(os.path.join(GOLD, "tiny_xl_euler.pt"))
    inp = g["inputs"]
    hw = inp["latents"].shape[2]
    eng = Engine(TINY_XL_CONFIG, hw, hw, device=0)
    eng.load_state_dict(random_state_dict(TINY_XL_CONFIG, seed=g["weight_seed"]))
    det, det_same = _ref_stream_against_plain(eng, inp, EulerTables(), 0, 12)
    sto, sto_same = _ref_stream_against_plain(eng, inp, EulerAncestralTables(), 31, 12)
    eng.close()
    print(f"reference stream vs plain pass, max |diff| per step: Euler {['%.2e' % d for d in det]} (bit-identical: {all(det_same)}); "
          f"Euler ancestral {['%.2e' % d for d in sto]} (bit-identical: {all(sto_same)})")
    if all(det_same):
        assert all(sto_same), sto
    else:
        for i, (d, s) in enumerate(zip(det, sto)):
            assert s <= 2 * d, (i, s, d)


# ------------------------------------------------------------------------------------------------ 5: the façades against the oracle loops
def test_region_diffusion_sde_matches_oracle_loop():
    from rich_text_to_image_amd.schedulers import DPMSolverTables
    g = torch.load(os.path.join(GOLD, "tiny_sd_plms.pt"))
    inp = g["inputs"]
    steps, seed = 8, 17
    h, w = inp["latents"].shape[2:]
    sd = random_state_dict(TINY_SD_CONFIG, seed=g["weight_seed"])
    masks = [x[None].repeat(1, 4, 1, 1) for x in inp["masks"]]
    tfd = {"word_pos": inp["word_pos"], "font_size": inp["font_size"]}
    m = _sd_model(g["weight_seed"], scheduler=DPMSolverTables(algorithm="sde-dpmsolver++"))
    m.masks = masks
    out = m.produce_latents(inp["embeds"], num_inference_steps=steps, guidance_scale=g["guidance_scale"], latents=inp["latents"].clone(),
                            text_format_dict=tfd, inject_selfattn=0.5, inject_background=0.3, noise_seed=seed)
    field = _device_field(seed, h, w)
    ref = region_loop.rich_loop_sd(OracleUNet(TINY_SD_CONFIG, sd), RefSdeDpmSolver(field), inp["embeds"], masks, inp["latents"], steps,
                                   g["guidance_scale"], tfd, 0.5, 0.3)
    r = rel_l2(out, ref)
    print(f"RegionDiffusion SDE-DPM-Solver++ order 2 vs oracle loop rel-L2 {r:.3e}")
    assert r < 3e-2
    emb2 = inp["embeds"][[0, -1]]
    out = m.plain_latents(emb2, num_inference_steps=steps, guidance_scale=g["guidance_scale"], latents=inp["latents"].clone(), noise_seed=seed)
    ref = region_loop.plain_loop(OracleUNet(TINY_SD_CONFIG, sd), RefSdeDpmSolver(field), emb2, inp["latents"], steps, g["guidance_scale"])
    r = rel_l2(out, ref)
    print(f"RegionDiffusion plain pass SDE-DPM-Solver++ order 2 vs oracle plain loop rel-L2 {r:.3e}")
    assert r < 3e-2


@pytest.mark.parametrize("kind", [EULER_A, SDE_2], ids=["euler_ancestral", "sde_dpm_2"])
def test_region_diffusion_xl_stochastic_matches_oracle_loop(kind):
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables
    g = torch.load(os.path.join(GOLD, "tiny_xl_euler.pt"))
    inp = g["inputs"]
    steps, seed, isa, ibg = 8, 23, 0.5, 0.3
    lh = inp["latents"].shape[2]
    hw = lh * 8
    sd = random_state_dict(TINY_XL_CONFIG, seed=g["weight_seed"])
    masks = [x[None].repeat(1, 4, 1, 1) for x in inp["masks"]]
    tfd = {"word_pos": inp["word_pos"], "font_size": inp["font_size"]}
    m = _xl_model(g["weight_seed"])
    m.scheduler = EulerAncestralTables() if kind == EULER_A else DPMSolverTables(algorithm="sde-dpmsolver++")      # the diffusers idiom
    assert m.scheduler.kind == kind
    m.masks = masks
    field = _device_field(seed, lh, lh)
    mk = (lambda: RefEulerAncestral(field)) if kind == EULER_A else (lambda: RefSdeDpmSolver(field))
    start = inp["latents"] * mk().set_timesteps(steps).init_noise_sigma                   # prepare_latents (xl.py:536) is the caller's job
    out = _xl_sample(m, inp, hw, steps, g["guidance_scale"], run_rich_text=True, text_format_dict=tfd, inject_selfattn=isa, inject_background=ibg,
                     noise_seed=seed)
    tid = torch.tensor([[hw * 1.0, hw * 1.0, 0, 0, hw * 1.0, hw * 1.0]])
    ref = region_loop.rich_loop_xl(OracleUNet(TINY_XL_CONFIG, sd), mk(), inp["embeds"], inp["pooled"], tid, masks, start, steps,
                                   g["guidance_scale"], tfd, isa, ibg)
    r = rel_l2(out, ref)
    print(f"RegionDiffusionXL kind {kind} ({isa}, {ibg}) vs oracle loop rel-L2 {r:.3e}")
    assert r < 3e-2
    out = _xl_sample(m, inp, hw, steps, g["guidance_scale"], run_rich_text=False, noise_seed=seed)      # the plain pass runs prompts 0 and 1
    added = {"text_embeds": inp["pooled"][:2], "time_ids": tid.repeat(2, 1)}
    ref = region_loop.plain_loop(OracleUNet(TINY_XL_CONFIG, sd), mk(), inp["embeds"][:2], start, steps, g["guidance_scale"], added=added, xl=True)
    r = rel_l2(out, ref)
    print(f"RegionDiffusionXL plain pass kind {kind} vs oracle plain loop rel-L2 {r:.3e}")
    assert r < 3e-2


# ------------------------------------------------------------------------------------------------ 6: the image start
def test_image_start_with_pinned_background():
    """Kind 6, strength 0.6 of 10 steps, keep_source = background on the tiny SD config with a hard partition as masks: the pinned
    pixels end as the source (the bound of tests/test_img2img_gpu.py at the level (1, 0)), and the loop equals the rich loop of
    oracle/region_loop.py restated with the pin at source_levels() after every iteration.  The noise index is the index in the EXECUTED
    schedule."""
    from rich_text_to_image_amd.schedulers import DPMSolverTables
    from tests.img2img_ref import blend_bound
    g = torch.load(os.path.join(GOLD, "tiny_sd_plms.pt"))
    inp = g["inputs"]
    n, strength, isa, ibg, seed, gs = 10, 0.6, 0.5, 0.3, 29, g["guidance_scale"]
    h, w = inp["latents"].shape[2:]
    sd = random_state_dict(TINY_SD_CONFIG, seed=g["weight_seed"])
    hard = torch.nn.functional.one_hot(inp["masks"][:, 0].argmax(0), inp["masks"].shape[0]).permute(2, 0, 1).float()     # [R, h, w]
    masks = [x[None, None].repeat(1, 4, 1, 1) for x in hard]
    keep = masks[-1][:, :1]
    assert 0.05 < keep.mean().item() < 0.95
    tfd = {"word_pos": inp["word_pos"], "font_size": inp["font_size"]}
    gen = torch.Generator().manual_seed(53)
    x0, noise = 0.8 * torch.randn(1, 4, h, w, generator=gen), torch.randn(1, 4, h, w, generator=gen)
    m = _sd_model(g["weight_seed"], scheduler=DPMSolverTables(algorithm="sde-dpmsolver++"))
    m.masks = masks
    out = m.produce_latents(inp["embeds"], num_inference_steps=n, guidance_scale=gs, text_format_dict=tfd, inject_selfattn=isa,
                            inject_background=ibg, image=x0.to(DEV), strength=strength, noise=noise.to(DEV), keep_source="background",
                            noise_seed=seed).cpu()
    # pinned pixels
    kept = keep.expand(1, 4, h, w) == 1
    bound = blend_bound(x0, x0, noise, 1.0, 0.0)
    err = (out.double() - x0.double()).abs()
    print(f"pinned pixels: max |err| {err[kept].max().item():.3e}, worst err / bound {(err[kept] / bound[kept]).max().item():.3f}")
    assert bool((err[kept] <= bound[kept]).all())
    # the loop
    sched = RefSdeDpmSolver(_device_field(seed, h, w), 2, strength=strength).set_timesteps(n)
    assert len(sched.timesteps) == 6 and len(m.scheduler.timesteps) == 6
    a, b = sched.start_level()
    lat = (a * x0.double() + b * noise.double()).float()
    lat_ref, levels, unet, k = lat.clone(), sched.source_levels(), OracleUNet(TINY_SD_CONFIG, sd), len(sched.timesteps)
    feats = 0
    for i, t in enumerate(sched.timesteps):
        feat = bool(t > (1 - isa) * 1000)
        feats += feat
        eu, et, eur, etr = region_loop.rich_step_forwards(unet, lat, lat_ref, t, inp["embeds"], lambda j: None, masks, tfd, True, feat)
        eps, eps_ref = eu + gs * (et - eu), eur + gs * (etr - eur)
        o = sched.step(torch.cat([eps, eps_ref]), t, torch.cat([lat, lat_ref]))["prev_sample"]
        lat, lat_ref = o[:1], o[1:]
        if i == int(ibg * k):
            lat = lat_ref * masks[-1] + lat * (1 - masks[-1])
        a, b = levels[i]
        lat = keep * (a * x0 + b * noise) + (1 - keep) * lat
    assert feats >= 1
    r = rel_l2(out, lat)
    print(f"image start, SDE-DPM-Solver++ order 2, strength {strength}, background pinned vs restated loop: rel-L2 {r:.3e}")
    assert r < 3e-2
    assert rel_l2(out[~kept], x0[~kept]) > 1e-2                 # the free pixels moved


# ------------------------------------------------------------------------------------------------ 7: split image
def test_sample_cli_split_image_sde_two_ranks_share_one_image(tmp_path):
    """`--gpus 2 --split_image --scheduler sde-dpmsolver++`: two ranks on one GPU over gloo; every rank sets the same noise seed and runs
    the epilogue on the full eps set, so both hold the same latents with nothing extra exchanged, and rank 0's image is byte-identical
    with the one-GPU run."""
    import subprocess
    import sys
    from rich_text_to_image_amd import sample
    from tests.test_checkpoint_gpu import _write_dir
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _write_dir(str(tmp_path / "ckpt"))
    ja = json.dumps({"ops": [{"insert": "a "}, {"attributes": {"link": "a wooden fence covered in snow"}, "insert": "fence"}, {"insert": " and a "},
                             {"attributes": {"font": "slabo"}, "insert": "barn"}, {"insert": " under a night sky\n"}]})
    (tmp_path / "a.json").write_text(ja)
    # 12 steps: the token-map hooks record from the 11th call on (n_maps > 10, rd.py:422)
    common = ["--load_path", str(tmp_path / "ckpt"), "--model", "SD", "--sample_steps", "12", "--num_segments", "4", "--inject_selfattn", "0.5",
              "--inject_background", "0.3", "--scheduler", "sde-dpmsolver++"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env.update(PYTHONPATH=root + os.pathsep + env.get("PYTHONPATH", ""), RTDIFF_DIST_BACKEND="gloo", RTDIFF_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "rich_text_to_image_amd.sample", "--gpus", "2", "--split_image", "--rich_text_json", str(tmp_path / "a.json"),
                        "--seeds", "3", "--run_dir", str(tmp_path / "out2")] + common, env=env, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "[rank 0] request 0 seed 3" in r.stdout and "[rank 1] request 0 seed 3" in r.stdout
    sample.main(["--rich_text_json", ja, "--seed", "3", "--run_dir", str(tmp_path / "out1")] + common)
    sample.main(["--rich_text_json", ja, "--seed", "3", "--run_dir", str(tmp_path / "out0")] + common[:-1] + ["dpmsolver++"])
    for kind in ("plain", "rich"):
        one = open(tmp_path / "out1" / f"seed3_{kind}.jpg", "rb").read()
        assert open(tmp_path / "out2" / f"seed3_{kind}.jpg", "rb").read() == one, kind
        assert open(tmp_path / "out0" / f"seed3_{kind}.jpg", "rb").read() != one, kind        # the flag reached the pipeline
