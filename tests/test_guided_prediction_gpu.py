"""The guided-prediction pre-pass on the GPU (csrc/guided.hip + step_driver.inl guided_prepass: CFG rescale and v-prediction in front of
the unchanged step epilogues) against the fp64 restatement of tests/guided_ref.py, without the UNet, every step; the rescale factor alone
through rt_op_guided_prediction; the reference pair as the plain pass; reproducibility; off = today; refusal; and both façades.

A tiny engine whose arena is only marked bound; seeded model outputs go straight into the eps slots of the step's streams, every other
slot holds NaN, then region_step_finish / plain_step_finish, exactly as tests/test_step_epilogue_gpu.py drives the epilogues."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict  # noqa: E402
from tests import guided_ref as G  # noqa: E402
from tests import step_ref as S  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
DEV = "cuda:0"
NAN = float("nan")
SEED = 41


def _engine(eng_hw, n_prompts, max_streams=8, max_prompts=8):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(TINY_SD_CONFIG, eng_hw[0], eng_hw[1], device=0, max_streams=max_streams, max_prompts=max_prompts)
    e.arena_mark_bound()
    g = torch.Generator().manual_seed(9)
    e.set_prompts(torch.randn(n_prompts, 77, TINY_SD_CONFIG["cross_attention_dim"], generator=g).to(DEV))
    return e


def _view(ptr, nfloat):
    from rich_text_to_image_amd.launcher import _DevicePointer
    return torch.as_tensor(_DevicePointer(ptr, nfloat * 4), device=DEV).view(torch.float32)


def _device_field(h, w):
    """The engine's own noise field, read back (the accuracy of the device normals does not enter)."""
    from rich_text_to_image_amd.engine import step_noise
    cache = {}

    def fn(i):
        if i not in cache:
            cache[i] = step_noise(SEED, i, h, w).cpu()
        return cache[i]
    return fn


class Run:
    """One pass over a case's schedule on engine `e`; `check` compares every step with the restatement."""

    def __init__(self, e, case, inputs, elide=None, defer=None, setting=None, ref_feed=None):
        self.e, self.c = e, case
        self.x, self.M, self.steps = inputs
        self.elide = case["elide"] if elide is None else elide
        self.defer = case["defer"] if defer is None else defer
        self.setting = (case["vpred"], case["phi"]) if setting is None else setting
        self.ref_feed = ref_feed
        h, w = case["lat"]
        self.hw = h * w
        self.field = _device_field(h, w)
        self.worst = dict(lat=0.0, lat_ref=0.0, noise_pred=0.0, trajectory=0.0)

    def sched(self):
        return G.make_sched(self.c["kind"], self.c["n"], noise_fn=self.field)

    @property
    def eps(self):
        from rich_text_to_image_amd.launcher import eps_tensor
        buf, per = eps_tensor(self.e)
        assert per == self.hw * 16
        return buf.view(torch.float32)

    def put(self, s, x):
        self.eps[s * self.hw * 4:(s + 1) * self.hw * 4].copy_(x.reshape(4, self.hw).t().reshape(-1))

    def step(self, i, ep):
        c, e = self.c, self.e
        self.eps.fill_(NAN)
        if c["mode"] == "plain":
            self.put(0, ep["u"].to(DEV)); self.put(1, ep["b"].to(DEV))
            torch.cuda.synchronize()                           # the engine launches on a stream of its own
            e.plain_step_finish(i, c["g"])
            return None
        p = S.plan(i, self.ts, c["R"], c["isa"], c["ibg"], c["xl"], self.elide)
        for s, role in enumerate(p["streams"]):
            if role in ("ur", "tr") and not p["step_ref"]:
                continue                                       # the pair's slots stay NaN on a step that does not step it
            self.put(s, ep[role].to(DEV))
        torch.cuda.synchronize()
        e.region_step_finish(i, c["g"], c["isa"], c["ibg"], c["xl"], elide=self.elide, defer_blend=self.defer)
        if self.defer:
            e.background_blend()
        return p

    def go(self, check=True):
        c, e = self.c, self.e
        h, w = c["lat"]
        vpred, phi = self.setting
        one, traj = self.sched(), self.sched()
        self.ts = one.timesteps
        e.set_schedule(G.KINDS[c["kind"]], one.timesteps, one.table(), c["n"])
        e.set_noise_seed(SEED)
        e.set_prediction(int(vpred), phi)
        e.set_latents(self.x.to(DEV))
        M64 = [m.double() for m in self.M]
        prev, prev_ref = (t.cpu().double() for t in e.read_latents(h, w, with_ref=True))
        t_lat, t_ref = prev.clone(), prev_ref.clone()
        lats, refs = [], []
        for i, ep in enumerate(self.steps):
            if self.ref_feed is not None:
                ep = dict(ep, ur=self.ref_feed[i]["u"], tr=self.ref_feed[i]["b"])
            p = self.step(i, ep)
            got, got_ref = (t.cpu() for t in e.read_latents(h, w, with_ref=True))
            lats.append(got); refs.append(got_ref)
            if check:
                ep64 = {k: v.double() for k, v in ep.items()}
                r = G.step_once(c, one, i, ep64, M64, prev, prev_ref, elide=self.elide)
                rt = G.step_once(c, traj, i, ep64, M64, t_lat, t_ref, elide=self.elide)
                t_lat = rt["lat"][0]
                npred = _view(e.state_ptrs()[1], 4 * self.hw).clone().cpu().reshape(1, 4, h, w)
                outs = {"lat": got}
                if p is not None:                              # the plain step keeps no noise_pred
                    t_ref = rt["lat_ref"][0]
                    outs.update(lat_ref=got_ref, noise_pred=npred)
                    if not p["step_ref"]:
                        assert torch.equal(got_ref.double(), prev_ref), (c["name"], i, "the unstepped reference latents moved")
                for k, g in outs.items():
                    assert torch.isfinite(g).all(), (c["name"], i, k, "a poisoned slot was read")
                    ratio = ((g.double() - r[k][0]).abs() / (S.ULPS * S.U32 * r[k][1])).max().item()
                    self.worst[k] = max(self.worst[k], ratio)
                    assert ratio <= 1.0, (c["name"], i, k, ratio)
                err = (got.double() - t_lat).abs().max().item() / (1e-5 * (i + 1) * t_lat.abs().max().item())
                self.worst["trajectory"] = max(self.worst["trajectory"], err)
                assert err <= 1.0, (c["name"], i, "trajectory", err)
                prev, prev_ref = got.double(), got_ref.double()
        return lats, refs


def _prepare(c):
    inputs = G.case_inputs(c)
    e = _engine(c["eng"], 2 if c["mode"] == "plain" else c["R"] + 1)
    if c["mode"] != "plain":
        e.set_masks([m.to(DEV) for m in inputs[1]])
    return e, inputs


# ------------------------------------------------------------------------------------------------ 1: every step against the restatement
@pytest.mark.parametrize("name", [c["name"] for c in G.CASES])
def test_every_step_matches_the_restatement(name):
    c = G.CASE[name]
    e, inputs = _prepare(c)
    try:
        run = Run(e, c, inputs)
        first, first_ref = run.go()
        print(f"{name}: worst error / bar  " + "  ".join(f"{k} {v:.3f}" for k, v in run.worst.items() if v or k == "lat"))
        # reproducibility: the same run twice gives equal bits
        again, again_ref = Run(e, c, inputs).go(check=False)
        assert all(torch.equal(a, b) for a, b in zip(first + first_ref, again + again_ref)), "second pass"
        if c["elide"]:
            full, _ = Run(e, c, inputs, elide=False).go(check=False)
            assert all(torch.equal(a, b) for a, b in zip(first, full)), "elide"
        if c["defer"]:
            fused, _ = Run(e, c, inputs, defer=False).go(check=False)
            assert all(torch.equal(a, b) for a, b in zip(first, fused)), "deferred blend"
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 2: the factor
# 96 x 96 = 36 workgroups: the finish kernel stages the partial sums 32 workgroups at a time, so this is its second trip
@pytest.mark.parametrize("h,w", [(24, 40), (16, 16), (12, 8), (96, 96)], ids=["960px", "256px", "96px", "9216px"])
def test_factor_is_within_one_ulp_of_the_fp64_factor(h, w):
    """Plain mode, g = 2, inputs multiples of 2^-8 in [-4, 4]: text and cfg = u + 2 (t - u) are exact in fp32 with or without
    contraction, and the sums of the kernel are exact in fp64 (37 bits); both factors within 1 fp32 ulp of the fp64 factor of those
    exact values, and the rescaled predictions are one fp32 product."""
    from rich_text_to_image_amd.engine import guided_prediction
    gen = torch.Generator().manual_seed(h * w)
    eps = (torch.randint(-1024, 1025, (4, h * w, 4), generator=gen).float() / 256).to(DEV)          # streams u, t, u_ref, t_ref
    lat = torch.zeros(1, 4, h, w, device=DEV)
    for phi in (0.7, 1.0):
        gp, fac = guided_prediction(eps, lat, 2.0, 0, 1, lat_ref=lat, s_uref=2, s_tref=3, plain=True, step_ref=True, guidance_rescale=phi)
        e64 = eps.cpu().double()
        for k, (u, t) in enumerate(((0, 1), (2, 3))):
            cfg = e64[u] + 2.0 * (e64[t] - e64[u])
            assert torch.equal(cfg.float().double(), cfg)
            p = G.phi32(phi)
            f = p * e64[t].std().item() / cfg.std().item() + (1.0 - p)
            f32 = torch.tensor(f, dtype=torch.float64).float()
            ulp = torch.nextafter(f32, torch.tensor(float("inf"))) - f32
            got = fac[k].cpu()
            print(f"{h}x{w} phi {phi} stream {k}: factor {got.item():.8f}, fp64 {f:.10f}, distance {abs(got.double().item() - f) / ulp.item():.3f} ulp")
            assert abs(got.double().item() - f) <= ulp.item(), (k, got.item(), f)
            assert torch.equal(gp[k].cpu(), cfg.float() * got)
    # phi = 0, epsilon: the composed values themselves, factors (1, 1); without a stepped pair slot 1 is not written and its factor is 0
    gp, fac = guided_prediction(eps, lat, 2.0, 0, 1, plain=True, prediction_type=1, cv=1.0, cx=0.0)
    assert torch.equal(gp[0].cpu(), (eps[0] + 2.0 * (eps[1] - eps[0])).cpu()) and torch.isnan(gp[1]).all() and fac.tolist() == [1.0, 0.0]


# ------------------------------------------------------------------------------------------------ 3: the pair is the plain pass
@pytest.mark.parametrize("kind", ["euler", "dpm2"])
def test_reference_pair_is_the_plain_pass(kind):
    """(v, 0.7): the pair's slots are fed the plain run's (u, t); lat_ref after every step equals the plain run's latents bit for bit -
    its own factor, its own latents in the conversion."""
    rich = G.CASE[f"{kind}_rich_v_phi"]
    plain = dict(rich, mode="plain", R=0, name=rich["name"] + "_as_plain")
    inputs = G.case_inputs(rich)
    e, _ = _prepare(rich)
    try:
        want, _ = Run(e, plain, inputs).go(check=False)
        feed = [dict(u=s["u"], b=s["b"]) for s in inputs[2]]
        # isa = 0.5 with ibg = 0: the pair is stepped on every step under both pipelines' rules, and nothing blends
        always = dict(rich, isa=0.5, ibg=0.0)
        _, refs = Run(e, always, inputs, ref_feed=feed).go(check=False)
        assert len(refs) == len(want) >= 6
        for i, (a, b) in enumerate(zip(refs, want)):
            assert torch.equal(a, b), (kind, i, (a - b).abs().max().item())
        assert (want[-1] - inputs[0]).abs().max().item() > 1e-2
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 4: off means today; refusal
def test_off_means_today_and_bad_values_are_refused():
    from rich_text_to_image_amd.engine import RtError
    c = dict(G.CASE["plms_rich_v_phi"])
    inputs = G.case_inputs(c)
    fresh, _ = _prepare(c)
    try:
        want = Run(fresh, c, inputs, setting=(False, 0.0)).go(check=False)
    finally:
        fresh.close()
    e, _ = _prepare(c)
    try:
        on = Run(e, c, inputs, setting=(True, 0.7)).go(check=False)
        assert not torch.equal(on[0][-1], want[0][-1])
        for bad in ((2, 0.0), (-1, 0.0), (0, 1.5), (1, -0.1)):
            with pytest.raises(RtError):
                e.set_prediction(*bad)
        with pytest.raises(ValueError):
            e.set_prediction("sample")
        again = Run(e, c, inputs, setting=(True, 0.7)).go(check=False)         # the refused calls changed nothing
        assert all(torch.equal(a, b) for a, b in zip(on[0] + on[1], again[0] + again[1]))
        e.set_prediction(0, 0.0)
        off = Run(e, c, inputs, setting=(False, 0.0)).go(check=False)
        assert all(torch.equal(a, b) for a, b in zip(off[0] + off[1], want[0] + want[1]))
    finally:
        e.close()


# ------------------------------------------------------------------------------------------------ 5: the façades
def _xl_model(seed, **kw):
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    return RegionDiffusionXL(device=0, unet_state_dict=random_state_dict(TINY_XL_CONFIG, seed=seed), config=TINY_XL_CONFIG, **kw)


def _xl_sample(m, inp, hw, steps, gs, **kw):
    return m.sample(prompt=None, height=hw, width=hw, num_inference_steps=steps, guidance_scale=gs, latents=inp["latents"].clone(),
                    prompt_embeds=inp["embeds"][1:], negative_prompt_embeds=inp["embeds"][:1], pooled_prompt_embeds=inp["pooled"][1:],
                    negative_pooled_prompt_embeds=inp["pooled"][:1], output_type="latent", original_size=(hw, hw), target_size=(hw, hw),
                    **kw).images


def test_xl_facade_honours_guidance_rescale():
    """Tiny SDXL config, real forwards, 4 steps.  Plain pass: sample(guidance_rescale=0.7) equals the engine-level loop with
    set_prediction(0, 0.7) and differs from phi = 0.  Rich pass: the pipeline attribute; equals the engine-level loop; its lat_ref
    trajectory equals the plain pass's under Euler, bit for bit, with and without the rescale; the call keyword keeps raising."""
    from rich_text_to_image_amd.schedulers import EulerTables
    g = torch.load(os.path.join(GOLD, "tiny_xl_euler.pt"))
    inp = g["inputs"]
    lh = inp["latents"].shape[2]
    hw, n, gs, isa = lh * 8, 4, 5.0, 0.5
    m = _xl_model(g["weight_seed"])
    base = _xl_sample(m, inp, hw, n, gs)
    out = _xl_sample(m, inp, hw, n, gs, guidance_rescale=0.7)
    assert torch.equal(_xl_sample(m, inp, hw, n, gs), base)                     # the next call does not keep the value
    rel = ((out - base).pow(2).sum() / base.pow(2).sum()).sqrt().item()
    print(f"plain pass, guidance_rescale 0.7 vs 0: rel-L2 {rel:.3e}")
    assert rel > 1e-3                                                            # fails where the argument is dropped
    assert torch.equal(_xl_sample(m, inp, hw, n, 1.0, guidance_rescale=0.7), _xl_sample(m, inp, hw, n, 1.0))      # only under CFG (xl.py:903)

    t = EulerTables().set_timesteps(n)
    tid = torch.tensor([[hw * 1.0, hw * 1.0, 0, 0, hw * 1.0, hw * 1.0]])
    lat0 = (inp["latents"] * t.init_noise_sigma).to(DEV)
    eng = m.unet.engine(lh, lh, streams=inp["embeds"].shape[0] + 2, prompts=inp["embeds"].shape[0])      # the façade's own engine

    def loop(phi, rich):
        eng.set_prompts(inp["embeds"].to(DEV), inp["pooled"].to(DEV), tid)          # the plain pass runs prompts 0 and 1
        eng.set_schedule(t.kind, t.timesteps.tolist(), t.table(), n)
        eng.set_prediction(0, phi)
        eng.set_latents(lat0)
        if rich:
            eng.set_masks(inp["masks"].repeat(1, 4, 1, 1).to(DEV))
            eng.set_fontsize(inp["word_pos"], inp["font_size"])
        traj = []
        for i in range(n):
            if rich:
                eng.region_step(i, gs, isa, 0.0, xl=True)
            else:
                eng.plain_step(i, gs)
            traj.append(eng.read_latents(lh, lh, with_ref=True))
        return traj

    assert torch.equal(loop(0.7, False)[-1][0], out)

    m.masks = [x[None].repeat(1, 4, 1, 1) for x in inp["masks"]]
    kx = dict(run_rich_text=True, text_format_dict={"word_pos": inp["word_pos"], "font_size": inp["font_size"]}, inject_selfattn=isa, inject_background=0.0)
    rich0 = _xl_sample(m, inp, hw, n, gs, **kx)
    with pytest.raises(NotImplementedError):
        _xl_sample(m, inp, hw, n, gs, guidance_rescale=0.7, **kx)
    m.guidance_rescale = 0.7
    rich = _xl_sample(m, inp, hw, n, gs, **kx)
    m.guidance_rescale = 0.0
    assert ((rich - rich0).pow(2).sum() / rich0.pow(2).sum()).sqrt().item() > 1e-3
    traj = loop(0.7, True)
    assert torch.equal(traj[-1][0], rich)
    # the pair against the plain pass whose two prompts are the pair's: [negative, base]
    def plain_of_pair(phi):
        eng.set_prompts(inp["embeds"][[0, -1]].to(DEV), inp["pooled"][[0, -1]].to(DEV), tid)
        eng.set_schedule(t.kind, t.timesteps.tolist(), t.table(), n)
        eng.set_prediction(0, phi)
        eng.set_latents(lat0)
        out = []
        for i in range(n):
            eng.plain_step(i, gs)
            out.append(eng.read_latents(lh, lh))
        return out
    same0 = all(torch.equal(a[1], b) for a, b in zip(loop(0.0, True), plain_of_pair(0.0)))
    same = [torch.equal(a[1], b) for a, b in zip(traj, plain_of_pair(0.7))]
    dist = [(a[1] - b).abs().max().item() for a, b in zip(traj, plain_of_pair(0.7))]
    print(f"rich pass lat_ref vs plain pass, phi 0.7: bit-identical {same} (without rescale: {same0}), max |diff| {['%.2e' % d for d in dist]}")
    assert same0 and all(same), (same0, dist)


def test_sd_facade_takes_guidance_rescale():
    """RegionDiffusion: `guidance_rescale=` on produce_latents / plain_latents (test_sd_string_entry_points_pass_guidance_rescale_on
    runs prompt_to_img and produce_attn_maps) equals the engine-level loop with set_prediction and differs from phi = 0; a v-prediction scheduler reaches the engine."""
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    from rich_text_to_image_amd.schedulers import PNDMTables
    g = torch.load(os.path.join(GOLD, "tiny_sd_plms.pt"))
    inp = g["inputs"]
    m = RegionDiffusion(0, unet_state_dict=random_state_dict(TINY_SD_CONFIG, seed=g["weight_seed"]), config=TINY_SD_CONFIG)
    m.masks = [x[None].repeat(1, 4, 1, 1) for x in inp["masks"]]
    kw = dict(num_inference_steps=4, guidance_scale=7.5, text_format_dict={"word_pos": inp["word_pos"], "font_size": inp["font_size"]},
              inject_selfattn=0.5, inject_background=0.5)
    base = m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), **kw)
    out = m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), guidance_rescale=0.7, **kw)
    assert ((out - base).pow(2).sum() / base.pow(2).sum()).sqrt().item() > 1e-3
    assert torch.equal(m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), **kw), base)
    m.guidance_rescale = 0.7
    assert torch.equal(m.produce_latents(inp["embeds"], latents=inp["latents"].clone(), **kw), out)
    m.guidance_rescale = 0.0
    h, w = inp["latents"].shape[2:]
    eng = m.unet.engine(h, w, streams=inp["embeds"].shape[0] + 2, prompts=inp["embeds"].shape[0], keys=77)
    t = PNDMTables().set_timesteps(4)
    eng.set_prompts(inp["embeds"].to(DEV))
    eng.set_masks([x.to(DEV) for x in m.masks])
    eng.set_fontsize(inp["word_pos"], inp["font_size"])
    eng.set_schedule(1, t.timesteps.tolist(), t.table(), 4)
    eng.set_prediction(0, 0.7)
    eng.set_latents(inp["latents"].to(DEV))
    for i in range(len(t.timesteps)):
        eng.region_step(i, 7.5, 0.5, 0.5, xl=False)
    assert torch.equal(eng.read_latents(h, w), out)
    emb2 = inp["embeds"][[0, -1]]
    p0 = m.plain_latents(emb2, num_inference_steps=4, guidance_scale=7.5, latents=inp["latents"].clone())
    p1 = m.plain_latents(emb2, num_inference_steps=4, guidance_scale=7.5, latents=inp["latents"].clone(), guidance_rescale=0.7)
    assert ((p1 - p0).pow(2).sum() / p0.pow(2).sum()).sqrt().item() > 1e-3
    m.scheduler = PNDMTables(prediction_type="v_prediction")
    pv = m.plain_latents(emb2, num_inference_steps=4, guidance_scale=7.5, latents=inp["latents"].clone())
    assert torch.isfinite(pv).all() and ((pv - p0).pow(2).sum() / p0.pow(2).sum()).sqrt().item() > 1e-2


def test_sd_string_entry_points_pass_guidance_rescale_on():
    """prompt_to_img(guidance_rescale=0.7) and produce_attn_maps(guidance_rescale=0.7) on a RegionDiffusion with a tokenizer, a text
    encoder and a VAE (tests/test_sample_gpu.py's tiny model): each differs from phi = 0 and equals the decoded latents of the
    engine-level loop with set_prediction(0, 0.7)."""
    from rich_text_to_image_amd.schedulers import PNDMTables
    from tests.test_sample_gpu import _model
    m = _model()
    n, gs, h, w = 4, 7.5, 64, 64
    g = torch.Generator().manual_seed(8)
    lat = torch.randn(1, 4, h, w, generator=g)
    masks = torch.softmax(torch.randn(2, 1, h, w, generator=g) * 2, 0).repeat(1, 4, 1, 1)
    m.masks = [masks[r:r + 1] for r in range(2)]
    prompts, neg = ["a wooden fence covered in snow", "a barn under a night sky"], ""
    kw = dict(num_inference_steps=n, guidance_scale=gs, latents=lat.clone(), inject_selfattn=0.5, inject_background=0.5)
    t = PNDMTables().set_timesteps(n)

    def engine_loop(emb, rich):
        eng = m.unet.engine(h, w, streams=emb.shape[0] + 2, prompts=emb.shape[0], keys=77)
        eng.set_prompts(emb.to(DEV))
        eng.set_fontsize(None, None)
        eng.set_schedule(1, t.timesteps.tolist(), t.table(), n)
        eng.set_prediction(0, 0.7)
        eng.set_latents(lat.to(DEV))
        if rich:
            eng.set_masks([x.to(DEV) for x in m.masks])
        for i in range(len(t.timesteps)):
            if rich:
                eng.region_step(i, gs, 0.5, 0.5, xl=False)
            else:
                eng.plain_step(i, gs)
        return m.latents_to_uint8(eng.read_latents(h, w))

    img0 = m.prompt_to_img(prompts, neg, **kw)
    img = m.prompt_to_img(prompts, neg, guidance_rescale=0.7, **dict(kw, latents=lat.clone()))
    assert img.shape == img0.shape == (1, 512, 512, 3) and (img != img0).any()
    assert (img == engine_loop(m.get_text_embeds(prompts, [neg]), True)).all()
    pkw = dict(num_inference_steps=n, guidance_scale=gs)
    att0 = m.produce_attn_maps(prompts[:1], neg, latents=lat.clone(), **pkw)
    att = m.produce_attn_maps(prompts[:1], neg, latents=lat.clone(), guidance_rescale=0.7, **pkw)
    assert (att != att0).any()
    assert (att == engine_loop(m.get_text_embeds(prompts[:1], [neg]), False)).all()
    assert (m.produce_attn_maps(prompts[:1], neg, latents=lat.clone(), **pkw) == att0).all()          # the value does not stick
