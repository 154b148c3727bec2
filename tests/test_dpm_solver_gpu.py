"""DPM-Solver++ on the GPU: the engine's DPM epilogue (csrc/step.hip step_epilogue_kernel<STEP_DPM> + step_driver.inl solver_coeffs / multistep_coeffs) against the
test-side restatement (tests/dpm_solver_ref.py), with and without the UNet; both façades against the oracle loops driven by the restated
scheduler; the split-image command line; and the default schedulers after a DPM run."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import region_loop  # noqa: E402
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict  # noqa: E402
from tests.dpm_solver_ref import RefDPMSolver, dpm_timesteps, scaled_linear_alphas_cumprod  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"


def rel_l2(a, b):
    a, b = a.float().cpu(), b.float().cpu()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


def _engine(hw, n_prompts):
    """A tiny engine for the epilogue alone: the UNet never runs, so its arena is only marked bound."""
    from rich_text_to_image_amd.engine import Engine
    e = Engine(TINY_SD_CONFIG, hw, hw, device=0)
    e.arena_mark_bound()
    g = torch.Generator().manual_seed(9)
    e.set_prompts(torch.randn(n_prompts, 77, TINY_SD_CONFIG["cross_attention_dim"], generator=g).to(DEV))
    return e


def _eps_slots(e, hw):
    from rich_text_to_image_amd.launcher import eps_tensor
    buf, per = eps_tensor(e)
    f = buf.view(torch.float32)
    n = per // 4
    return lambda s, x: f[s * n:(s + 1) * n].copy_(x.reshape(4, hw * hw).t().reshape(-1))      # NCHW [1,4,h,w] -> the stream's NHWC slot


def _set_dpm(e, order, n):
    ts = dpm_timesteps(n)
    e.set_schedule(3 if order == 2 else 2, [float(t) for t in ts], scaled_linear_alphas_cumprod().tolist(), n)
    return ts


@pytest.mark.parametrize("order", [1, 2])
@pytest.mark.parametrize("mode", ["sd", "xl", "plain"])
def test_epilogue_alone_matches_the_restatement(mode, order):
    """Seeded noise predictions written straight into the eps buffer of every stream, then the step's finish: region mask combine + CFG
    + DPM update of both streams + blend, against the fp32 restatement driven by the same CFG-combined predictions, every step."""
    hw, n, R, gs = 32, 20, 3, 7.5
    isa, ibg = (0.5, 0.3) if mode == "sd" else (0.0, 0.3)
    xl = mode == "xl"
    e = _engine(hw, 2 if mode == "plain" else R + 1)
    g = torch.Generator().manual_seed(4)
    masks = torch.softmax(torch.randn(R, 1, hw, hw, generator=g) * 2, 0).repeat(1, 4, 1, 1)
    if mode != "plain":
        e.set_masks([masks[r:r + 1].to(DEV) for r in range(R)])
    ts = _set_dpm(e, order, n)
    lat0 = torch.randn(1, 4, hw, hw, generator=g)
    e.set_latents(lat0.to(DEV))
    put = _eps_slots(e, hw)
    ref = RefDPMSolver(order).set_timesteps(n)
    assert ref.timesteps.tolist() == ts.tolist()
    lat, lat_ref = lat0.clone(), lat0.clone()
    M = [masks[r:r + 1] for r in range(R)]
    for i, t in enumerate(ts.tolist()):
        if mode == "plain":
            eu, et = torch.randn(1, 4, hw, hw, generator=g), torch.randn(1, 4, hw, hw, generator=g)
            put(0, eu.to(DEV)); put(1, et.to(DEV))
            e.plain_step_finish(i, gs)
            lat = ref.step(eu + gs * (et - eu), t, lat)["prev_sample"]
        else:
            F = 4 + R - 1                                    # uncond, base, uncond_ref, text_ref, regions (no elision: the pair always runs)
            ep = [torch.randn(1, 4, hw, hw, generator=g) for _ in range(F)]
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
        got, got_ref = e.read_latents(hw, hw, with_ref=True)
        bar = 1e-5 * (i + 1) * lat.abs().max().item()
        err = (got.cpu() - lat).abs().max().item()
        assert err <= bar, (mode, order, i, err, bar)
        if mode != "plain":
            assert (got_ref.cpu() - lat_ref).abs().max().item() <= 1e-5 * (i + 1) * lat_ref.abs().max().item(), (i, "reference stream")
    print(f"{mode} order {order}: last-step L-inf {err:.3e} (bar {bar:.3e})")
    e.close()


def _engine_ode(n, order, hw=32, c=2.0):
    """Plain mode, g = 1: each step reads the latents back and writes the exact noise prediction of data ~ N(0, c^2) into both slots."""
    e = _engine(hw, 2)
    ts = _set_dpm(e, order, n)
    x_T = torch.linspace(-3, 3, 4 * hw * hw).reshape(1, 4, hw, hw)
    e.set_latents(x_T.to(DEV))
    put = _eps_slots(e, hw)
    ref = RefDPMSolver(order).set_timesteps(n)
    a, s = ref.alpha_t, ref.sigma_t
    var = lambda t: a[t] ** 2 * c * c + s[t] ** 2
    x_ref = x_T.clone()
    for i, t in enumerate(ts.tolist()):
        x = e.read_latents(hw, hw)
        eps = s[t].to(DEV) * x / var(t).to(DEV)
        put(0, eps); put(1, eps)
        e.plain_step_finish(i, 1.0)
        x_ref = ref.step(s[t] * x_ref / var(t), t, x_ref)["prev_sample"]
    got = e.read_latents(hw, hw).cpu()
    e.close()
    a64, s64 = a.double(), s.double()
    var64 = lambda t: a64[t] ** 2 * c * c + s64[t] ** 2
    exact = x_T.double() * torch.sqrt(var64(0)) / torch.sqrt(var64(int(ts[0])))
    return got, x_ref, (got.double() - exact).abs().max().item()


def test_analytic_ode_through_the_engine():
    errs = []
    for n in (16, 32, 64, 128):
        got, x_ref, err = _engine_ode(n, 2)
        assert (got - x_ref).abs().max().item() <= 1e-5 * x_ref.abs().max().item(), n
        errs.append(err)
    ratios = [errs[k] / errs[k + 1] for k in range(3)]
    print("engine order-2 error ratios", ratios)
    assert all(r >= 2.8 for r in ratios), ratios
    got, x_ref, e1 = _engine_ode(64, 1)
    assert (got - x_ref).abs().max().item() <= 1e-5 * x_ref.abs().max().item()
    assert e1 >= 5 * errs[2], (e1, errs[2])


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


@pytest.mark.parametrize("order", [1, 2])
def test_region_diffusion_dpm_matches_oracle_loop(order):
    from rich_text_to_image_amd.schedulers import DPMSolverTables
    g = torch.load(os.path.join(GOLD, "tiny_sd_plms.pt"))
    inp = g["inputs"]
    steps = 8
    sd = random_state_dict(TINY_SD_CONFIG, seed=g["weight_seed"])
    masks = [x[None].repeat(1, 4, 1, 1) for x in inp["masks"]]
    tfd = {"word_pos": inp["word_pos"], "font_size": inp["font_size"]}
    m = _sd_model(g["weight_seed"], scheduler=DPMSolverTables(solver_order=order))
    m.masks = masks
    out = m.produce_latents(inp["embeds"], num_inference_steps=steps, guidance_scale=g["guidance_scale"], latents=inp["latents"].clone(),
                            text_format_dict=tfd, inject_selfattn=0.5, inject_background=0.3)
    ref = region_loop.rich_loop_sd(OracleUNet(TINY_SD_CONFIG, sd), RefDPMSolver(order), inp["embeds"], masks, inp["latents"], steps,
                                   g["guidance_scale"], tfd, 0.5, 0.3)
    r = rel_l2(out, ref)
    print(f"RegionDiffusion DPM-Solver++ order {order} vs oracle loop rel-L2 {r:.3e}")
    assert r < 3e-2
    # the plain (token-map) pass
    emb2 = inp["embeds"][[0, -1]]
    out = m.plain_latents(emb2, num_inference_steps=steps, guidance_scale=g["guidance_scale"], latents=inp["latents"].clone())
    ref = region_loop.plain_loop(OracleUNet(TINY_SD_CONFIG, sd), RefDPMSolver(order), emb2, inp["latents"], steps, g["guidance_scale"])
    r = rel_l2(out, ref)
    print(f"RegionDiffusion plain pass DPM-Solver++ order {order} vs oracle plain loop rel-L2 {r:.3e}")
    assert r < 3e-2


@pytest.mark.parametrize("isa,ibg", [(0.5, 0.3), (0.0, 0.5)], ids=["inject", "reference_stops"])
def test_region_diffusion_xl_dpm_matches_oracle_loop(isa, ibg):
    from rich_text_to_image_amd.schedulers import DPMSolverTables
    g = torch.load(os.path.join(GOLD, "tiny_xl_euler.pt"))
    inp = g["inputs"]
    steps, hw = 8, inp["latents"].shape[2] * 8
    sd = random_state_dict(TINY_XL_CONFIG, seed=g["weight_seed"])
    masks = [x[None].repeat(1, 4, 1, 1) for x in inp["masks"]]
    tfd = {"word_pos": inp["word_pos"], "font_size": inp["font_size"]}
    m = _xl_model(g["weight_seed"])
    m.scheduler = DPMSolverTables()                       # the diffusers idiom
    m.masks = masks
    out = _xl_sample(m, inp, hw, steps, g["guidance_scale"], run_rich_text=True, text_format_dict=tfd, inject_selfattn=isa, inject_background=ibg)
    tid = torch.tensor([[hw * 1.0, hw * 1.0, 0, 0, hw * 1.0, hw * 1.0]])
    ref = region_loop.rich_loop_xl(OracleUNet(TINY_XL_CONFIG, sd), RefDPMSolver(), inp["embeds"], inp["pooled"], tid, masks, inp["latents"],
                                   steps, g["guidance_scale"], tfd, isa, ibg)
    r = rel_l2(out, ref)
    print(f"RegionDiffusionXL DPM-Solver++ ({isa}, {ibg}) vs oracle loop rel-L2 {r:.3e}")
    assert r < 3e-2
    if isa == 0.5:
        out = _xl_sample(m, inp, hw, steps, g["guidance_scale"], run_rich_text=False)      # the plain pass runs prompts 0 and 1
        added = {"text_embeds": inp["pooled"][:2], "time_ids": tid.repeat(2, 1)}
        ref = region_loop.plain_loop(OracleUNet(TINY_XL_CONFIG, sd), RefDPMSolver(), inp["embeds"][:2], inp["latents"], steps,
                                     g["guidance_scale"], added=added, xl=True)
        r = rel_l2(out, ref)
        print(f"RegionDiffusionXL plain pass DPM-Solver++ vs oracle plain loop rel-L2 {r:.3e}")
        assert r < 3e-2


@pytest.mark.parametrize("xl", [False, True], ids=["sd", "xl"])
def test_colour_guided_dpm_loop_matches_oracle_loop(xl):
    from oracle.vae import TINY_VAE_CONFIG, OracleVAEDecoder, random_vae_state_dict
    from rich_text_to_image_amd.engine import VaeDecoder
    from rich_text_to_image_amd.schedulers import DPMSolverTables
    g = torch.load(os.path.join(GOLD, "tiny_xl_euler.pt" if xl else "tiny_sd_plms.pt"))
    inp = g["inputs"]
    cfg = TINY_XL_CONFIG if xl else TINY_SD_CONFIG
    hw = 128 if xl else 64
    sd = random_state_dict(cfg, seed=g["weight_seed"])
    vsd = random_vae_state_dict(TINY_VAE_CONFIG, seed=2)
    gen = torch.Generator().manual_seed(7)
    R = g["R"]
    lat = torch.randn(1, 4, hw, hw, generator=gen)
    m = torch.softmax(torch.randn(R, 1, hw, hw, generator=gen) * 2, 0).repeat(1, 4, 1, 1)
    masks = [m[r:r + 1] for r in range(R)]
    cm = [torch.rand(1, 1, 8 * hw, 8 * hw, generator=gen).repeat(1, 4, 1, 1) for _ in range(2)]
    tfd = {"word_pos": inp["word_pos"], "font_size": inp["font_size"], "target_RGB": [torch.rand(1, 3, 1, 1, generator=gen) for _ in range(2)],
           "guidance_start_step": 999, "color_guidance_weight": 0.5, "color_obj_atten": cm,
           "color_obj_atten_all": torch.rand(1, 4, hw, hw, generator=gen)}
    steps, gs, isa, ibg = 3, 6.0, 0.5, 0.5
    guidance = {"vae": OracleVAEDecoder(TINY_VAE_CONFIG, vsd), "scaling": TINY_VAE_CONFIG["scaling_factor"]}
    vae = VaeDecoder(TINY_VAE_CONFIG, hw, hw, device=0, state_dict=vsd)
    if xl:
        tid = torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]])
        ref = region_loop.rich_loop_xl(OracleUNet(cfg, sd), RefDPMSolver(), inp["embeds"], inp["pooled"], tid, masks, lat, steps, gs, tfd, isa, ibg,
                                       use_guidance=True, guidance=guidance)
        mdl = _xl_model(g["weight_seed"], vae=vae, vae_scaling_factor=TINY_VAE_CONFIG["scaling_factor"], scheduler=DPMSolverTables())
        mdl.masks = masks
        run = lambda guided: mdl.sample(prompt=None, height=8 * hw, width=8 * hw, num_inference_steps=steps, guidance_scale=gs, latents=lat.clone(),
                                        prompt_embeds=inp["embeds"][1:], negative_prompt_embeds=inp["embeds"][:1], pooled_prompt_embeds=inp["pooled"][1:],
                                        negative_pooled_prompt_embeds=inp["pooled"][:1], output_type="latent", run_rich_text=True, text_format_dict=tfd,
                                        use_guidance=guided, inject_selfattn=isa, inject_background=ibg).images
    else:
        ref = region_loop.rich_loop_sd(OracleUNet(cfg, sd), RefDPMSolver(), inp["embeds"], masks, lat, steps, gs, tfd, isa, ibg,
                                       use_guidance=True, guidance=guidance)
        mdl = _sd_model(g["weight_seed"], vae=vae, scheduler=DPMSolverTables())
        mdl.masks = masks
        run = lambda guided: mdl.produce_latents(inp["embeds"], num_inference_steps=steps, guidance_scale=gs, latents=lat.clone(), text_format_dict=tfd,
                                                 use_guidance=guided, inject_selfattn=isa, inject_background=ibg)
    out = run(True)
    assert rel_l2(run(False), out) > 1e-4                 # the guidance step really ran
    r = rel_l2(out, ref)
    print(f"colour-guided DPM-Solver++ loop ({'xl' if xl else 'sd'}) vs oracle: rel-L2 {r:.3e}")
    assert r < 3e-2


def test_default_schedulers_after_a_dpm_run_are_untouched():
    """A DPM run, then the default scheduler on the same object: the same latents as a fresh object (the history reset is complete)."""
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerTables, PNDMTables
    g = torch.load(os.path.join(GOLD, "tiny_sd_plms.pt"))
    inp = g["inputs"]
    masks = [x[None].repeat(1, 4, 1, 1) for x in inp["masks"]]
    kw = dict(num_inference_steps=6, guidance_scale=7.5, text_format_dict={"word_pos": inp["word_pos"], "font_size": inp["font_size"]},
              inject_selfattn=0.5, inject_background=0.5)
    fresh = _sd_model(g["weight_seed"])
    fresh.masks = masks
    want = fresh.produce_latents(inp["embeds"], latents=inp["latents"].clone(), **kw)
    m = _sd_model(g["weight_seed"], scheduler=DPMSolverTables())
    m.masks = masks
    dpm = m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), **kw)
    assert rel_l2(dpm, want) > 1e-3
    m.scheduler = PNDMTables()
    assert torch.equal(m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), **kw), want)
    with pytest.raises(ValueError):                        # SD-v1.5 runs PNDM or DPM-Solver++ only
        m.scheduler = EulerTables()
        m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), **kw)

    gx = torch.load(os.path.join(GOLD, "tiny_xl_euler.pt"))
    ix = gx["inputs"]
    hw = ix["latents"].shape[2] * 8
    kx = dict(run_rich_text=True, text_format_dict={"word_pos": ix["word_pos"], "font_size": ix["font_size"]}, inject_selfattn=0.5, inject_background=0.5)
    mx = [x[None].repeat(1, 4, 1, 1) for x in ix["masks"]]
    fresh = _xl_model(gx["weight_seed"])
    fresh.masks = mx
    want = _xl_sample(fresh, ix, hw, 6, 5.0, **kx)
    m = _xl_model(gx["weight_seed"], scheduler=DPMSolverTables(solver_order=1))
    m.masks = mx
    assert rel_l2(_xl_sample(m, ix, hw, 6, 5.0, **kx), want) > 1e-3
    m.scheduler = EulerTables()
    assert torch.equal(_xl_sample(m, ix, hw, 6, 5.0, **kx), want)


def test_sample_cli_split_image_dpm_two_ranks_share_one_image(tmp_path):
    """`--gpus 2 --split_image --scheduler dpmsolver++`: two ranks on one GPU over gloo (as tests/test_checkpoint_gpu.py does); every rank
    runs the epilogue on the full eps set, so both hold the same history, and rank 0's image is byte-identical with the one-GPU run."""
    import subprocess
    import sys
    from rich_text_to_image_amd import sample
    from tests.test_checkpoint_gpu import _write_dir
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    _write_dir(str(tmp_path / "ckpt"))
    ja = json.dumps({"ops": [{"insert": "a "}, {"attributes": {"link": "a wooden fence covered in snow"}, "insert": "fence"}, {"insert": " and a "},
                             {"attributes": {"font": "slabo"}, "insert": "barn"}, {"insert": " under a night sky\n"}]})
    (tmp_path / "a.json").write_text(ja)
    # 12 steps: the token-map hooks record from the 11th call on (n_maps > 10, rd.py:422); 10 DPM steps would leave no maps
    common = ["--load_path", str(tmp_path / "ckpt"), "--model", "SD", "--sample_steps", "12", "--num_segments", "4", "--inject_selfattn", "0.5",
              "--inject_background", "0.3", "--scheduler", "dpmsolver++"]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env.update(PYTHONPATH=root + os.pathsep + env.get("PYTHONPATH", ""), RTDIFF_DIST_BACKEND="gloo", RTDIFF_FORCE_DEVICE="0", HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "rich_text_to_image_amd.sample", "--gpus", "2", "--split_image", "--rich_text_json", str(tmp_path / "a.json"),
                        "--seeds", "3", "--run_dir", str(tmp_path / "out2")] + common, env=env, capture_output=True, text=True, timeout=900, cwd=str(tmp_path))
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-3000:]
    assert "[rank 0] request 0 seed 3" in r.stdout and "[rank 1] request 0 seed 3" in r.stdout
    sample.main(["--rich_text_json", ja, "--seed", "3", "--run_dir", str(tmp_path / "out1")] + common)
    sample.main(["--rich_text_json", ja, "--seed", "3", "--run_dir", str(tmp_path / "out0")] + common[:-2])
    for kind in ("plain", "rich"):
        one = open(tmp_path / "out1" / f"seed3_{kind}.jpg", "rb").read()
        assert open(tmp_path / "out2" / f"seed3_{kind}.jpg", "rb").read() == one, kind
        assert open(tmp_path / "out0" / f"seed3_{kind}.jpg", "rb").read() != one, kind        # the flag reached the pipeline
