"""Request isolation one layer above the engine: a request on a pipeline object that has served other requests equals the same request
on a pipeline nothing else has used, bit for bit (torch.equal), and the serving path `sample --requests FILE` writes the same bytes
for a request whatever lines stand in front of it.  The sticky state of the facades is listed in INTEGRATION.md ("State that outlives
a run"); a request below carries everything the inventory calls per request (its scheduler object, its masks, its keywords) and the
histories return every pipeline attribute they set by the documented call (disable_freeu, clear_image_prompts, guidance_rescale = 0).
The engine level is tests/test_request_isolation_gpu.py."""
import json

import pytest
import torch

pytestmark = pytest.mark.gpu

import isolation_cases as I  # noqa: E402
from ip_adapter_ref import synthetic_checkpoint  # noqa: E402
from isolation_cases import FU  # noqa: E402
from oracle.vae import TINY_VAE_CONFIG, random_vae_state_dict  # noqa: E402


def _tables(name, **kw):
    from rich_text_to_image_amd import schedulers as S
    return {"euler": S.EulerTables, "euler-a": S.EulerAncestralTables, "pndm": S.PNDMTables,
            "dpm1": lambda: S.DPMSolverTables(solver_order=1), "dpm2": lambda: S.DPMSolverTables(solver_order=2),
            "sde2": lambda: S.DPMSolverTables(solver_order=2, algorithm="sde-dpmsolver++")}[name](**kw)


class Pipe:
    """One pipeline object of a family ("xl": RegionDiffusionXL.sample, "sd": RegionDiffusion.produce_latents / plain_latents) with the
    tiny VAE and a synthetic IP-Adapter, and the requests of this module on it."""

    def __init__(self, which, cases):
        from rich_text_to_image_amd.engine import VaeDecoder
        from rich_text_to_image_amd.region_diffusion import RegionDiffusion
        from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
        self.which, self.c = which, cases
        c = cases["probe"]
        sd = {k: v for k, v in c["sd"].items() if "_ip." not in k}
        vae = VaeDecoder(TINY_VAE_CONFIG, c["h"], c["w"], device=0, state_dict=random_vae_state_dict(TINY_VAE_CONFIG, seed=2))
        if which == "xl":
            self.m = RegionDiffusionXL(device=0, unet_state_dict=sd, config=c["cfg"], vae=vae, vae_scaling_factor=TINY_VAE_CONFIG["scaling_factor"])
        else:
            self.m = RegionDiffusion(0, unet_state_dict=sd, config=c["cfg"], vae=vae)
        self.m.load_ip_adapter(synthetic_checkpoint(c["cfg"], sd, T=4, E=24, seed=5)[0])

    def request(self, c, scheduler, *, R=3, rich=True, steps=3, keys=77, key_counts=None, font=True, **kw):
        """One request: its scheduler object, its masks and its keywords travel with it, as sample.generate hands them over."""
        m = self.m
        m.scheduler = _tables(scheduler)
        m.masks = [c["masks"][R][r:r + 1] for r in range(R)]
        rows = list(range(1, R + 1)) if rich else [R]
        tfd = dict(kw.pop("tfd", {}))
        if font:
            tfd.update(word_pos=c["wp"], font_size=c["fs"])
        start = {} if "image" in kw else {"latents": c["noise"].clone()}
        if self.which == "xl":
            counts = {} if key_counts is None else dict(prompt_key_counts=[key_counts[r] for r in rows], negative_key_counts=[key_counts[0]])
            return m.sample(prompt=None, height=8 * c["h"], width=8 * c["w"], num_inference_steps=steps, guidance_scale=c["gs"],
                            prompt_embeds=c["emb"][rows, :keys], negative_prompt_embeds=c["emb"][:1, :77], pooled_prompt_embeds=c["pooled"][rows],
                            negative_pooled_prompt_embeds=c["pooled"][:1], output_type="latent", run_rich_text=rich, text_format_dict=tfd,
                            inject_selfattn=c["isa"] if rich else 0, inject_background=c["ibg"] if rich else 0, **counts, **start, **kw).images.clone()
        emb = c["emb"][[0] + rows, :keys]
        counts = None if key_counts is None else [key_counts[r] for r in [0] + rows]
        if rich:
            return m.produce_latents(emb, height=8 * c["h"], width=8 * c["w"], num_inference_steps=steps, guidance_scale=c["gs"], text_format_dict=tfd,
                                     inject_selfattn=c["isa"], inject_background=c["ibg"], key_counts=counts, **start, **kw).clone()
        return m.plain_latents(emb, 8 * c["h"], 8 * c["w"], steps, c["gs"], key_counts=counts, **start, **kw).clone()

    # the two probe requests of a family: a rich loop on the default sampler, and a plain pass on a stochastic sampler without a seed
    def probe_rich(self):
        return self.request(self.c["probe"], "euler" if self.which == "xl" else "pndm", steps=3 if self.which == "xl" else 4)

    def probe_plain(self):
        return self.request(self.c["probe"], "euler-a" if self.which == "xl" else "sde2", rich=False)


def _cases(which):
    c = dict(probe=I.make_case(which), other=I.make_case(which, seed=101), wide=I.make_case(which, 32, 48, seed=103))
    g = torch.Generator().manual_seed(9)
    o = c["other"]                                        # eight regions = nine prompts: more than the seven a case carries
    D = o["emb"].shape[2]
    o["emb9"] = torch.randn(9, 231, D, generator=g)
    o["pooled9"] = torch.randn(9, 32, generator=g)
    o["masks"][8] = torch.softmax(torch.randn(8, 1, o["h"], o["w"], generator=g) * 2, 0).repeat(1, 4, 1, 1)
    c["eight"] = dict(o, emb=o["emb9"], pooled=o["pooled9"])
    c["eA"], c["tB"] = torch.randn(24, generator=g), torch.randn(3, D, generator=g)
    h, w = o["h"], o["w"]
    c["colour"] = {"target_RGB": [torch.rand(1, 3, 1, 1, generator=g) for _ in range(2)], "guidance_start_step": 999, "color_guidance_weight": 0.5,
                   "color_obj_atten": [torch.rand(1, 1, 8 * h, 8 * w, generator=g).repeat(1, 4, 1, 1) for _ in range(2)],
                   "color_obj_atten_all": torch.rand(1, 4, h, w, generator=g)}
    return c


# ---------------------------------------------------------------------------------------------------------------- the histories
def _default(p):
    return "euler" if p.which == "xl" else "pndm"


def r_other_schedulers(p):
    o = p.c["other"]
    for name in ("dpm1", "dpm2"):
        p.request(o, name)
    p.request(o, "sde2", noise_seed=5)
    if p.which == "xl":
        p.request(o, "euler-a", noise_seed=5, rich=False)
    else:
        p.request(o, "sde2", noise_seed=5, rich=False)


def r_noise_seed(p):
    """The probe's own stochastic plain pass with a seed: the next request passes none."""
    p.request(p.c["probe"], "euler-a" if p.which == "xl" else "sde2", rich=False, noise_seed=5)


def r_freeu(p):
    """The pipeline's attribute, then the UNet object's own (diffusers' unet.enable_freeu), each returned by its disable_freeu()."""
    p.m.enable_freeu(*FU)
    on = p.request(p.c["probe"], _default(p), steps=3 if p.which == "xl" else 4)
    p.m.disable_freeu()
    p.m.unet.enable_freeu(*FU)
    assert torch.equal(p.request(p.c["probe"], _default(p), steps=3 if p.which == "xl" else 4), on)
    p.m.unet.disable_freeu()
    return on


def r_image_prompts(p):
    p.m.set_image_prompts(base=dict(embeds=p.c["eA"], scale=0.9), regions={0: dict(tokens=p.c["tB"], scale=-0.7)})
    on = p.request(p.c["probe"], _default(p), steps=3 if p.which == "xl" else 4)
    p.request(p.c["other"], _default(p), rich=False)
    p.m.clear_image_prompts()
    return on


def r_long_prompt(p):
    """max_prompt_chunks = 3: prompts of up to 231 keys; the pipeline rebuilds its engines with room for them and keeps them."""
    kw = dict(max_prompt_chunks=3) if p.which == "xl" else {}
    p.request(p.c["other"], _default(p), keys=231, key_counts=[77, 231, 154, 231], **kw)
    assert p.m.unet.max_keys == 231


def r_image_start(p):
    o = p.c["other"]
    p.request(o, _default(p), steps=6, image=o["x0"], strength=0.7, noise=o["noise"], keep_source=o["keep"])


def r_guidance_rescale(p):
    o = p.c["other"]
    p.request(o, _default(p), rich=False, guidance_rescale=0.7)
    if p.which == "xl":                                   # the rich pass takes it as the pipeline attribute (its keyword raises, as in the reference)
        p.m.guidance_rescale = 0.5
        p.request(o, _default(p))
        p.m.guidance_rescale = 0.0
    else:
        p.request(o, _default(p), guidance_rescale=0.5)


def r_colour_guidance(p):
    p.request(p.c["other"], _default(p), use_guidance=True, tfd=p.c["colour"])


def r_eight_regions(p):
    """11 batched forwards and 9 prompts: the pipeline rebuilds its engines with room for them (as test_many_regions_grow_the_engine)."""
    p.request(p.c["eight"], _default(p), R=8)
    assert p.m.unet.max_streams >= 11 and p.m.unet.max_prompts >= 9


def r_other_size(p):
    p.request(p.c["wide"], _default(p))
    p.request(p.c["wide"], _default(p), rich=False)


def r_raises_part_way(p):
    """Requests that stop after the engine has been touched: a font-size word beyond the prompt's keys (refused by set_fontsize, behind
    set_prompts), a keep mask of the wrong shape (behind the engine lookup and the truncated schedule) and - where the pipeline takes a
    callback - an image start with a keep mask whose callback raises after the first step, which leaves the source in the engine."""
    from rich_text_to_image_amd.engine import RtError
    o = p.c["other"]
    with pytest.raises(RtError):
        p.request(o, _default(p), font=False, tfd={"word_pos": torch.tensor([3, 400]), "font_size": torch.tensor([2.0, 2.0])})
    with pytest.raises(ValueError):
        p.request(o, _default(p), steps=6, image=o["x0"], strength=0.7, noise=o["noise"], keep_source=o["keep"][:, :5])
    with pytest.raises(ValueError):                       # region 5 of a request with two region prompts: refused before any launch
        p.m.set_image_prompts(regions={5: dict(tokens=p.c["tB"])})
        try:
            p.request(o, _default(p))
        finally:
            p.m.clear_image_prompts()
    if p.which == "xl":
        class Stop(Exception):
            pass

        def stop(i, t, latents):
            raise Stop
        with pytest.raises(Stop):
            p.request(o, "dpm2", steps=6, image=o["x0"], strength=0.7, noise=o["noise"], keep_source=o["keep"], callback=stop)


REQUESTS = {"other-scheduler-objects": r_other_schedulers, "a-noise-seed": r_noise_seed, "freeu-enabled-then-disabled": r_freeu,
            "image-prompts-set-then-cleared": r_image_prompts, "max-prompt-chunks-3": r_long_prompt, "image-strength-keep-source": r_image_start,
            "guidance-rescale": r_guidance_rescale, "colour-guidance": r_colour_guidance, "eight-regions-grow-the-engine": r_eight_regions,
            "another-height-and-width": r_other_size, "a-request-that-raises-part-way": r_raises_part_way}


@pytest.fixture(scope="module", params=["xl", "sd"])
def served(request):
    """(the pipeline that serves every request of this module, the probes' results on pipelines nothing else has used)."""
    which = request.param
    cases = _cases(which)
    fresh = []
    for _ in range(2):
        p = Pipe(which, cases)
        fresh.append((p.probe_rich(), p.probe_plain()))
        del p
    yield Pipe(which, cases), fresh


def test_two_fresh_pipelines_agree(served):
    _, fresh = served
    for k, name in enumerate(("rich probe", "plain probe")):
        assert torch.equal(fresh[0][k], fresh[1][k]), f"two fresh pipelines differ in the {name}"
        assert bool(torch.isfinite(fresh[0][k]).all())


def _check(p, fresh, after):
    for name, got, want in (("rich probe", p.probe_rich(), fresh[0][0]), ("plain probe (stochastic, no seed)", p.probe_plain(), fresh[0][1])):
        if not torch.equal(got, want):
            pytest.fail(f"{p.which}: the {name} after [{after}] differs from a fresh pipeline (max |difference| {(got - want).abs().max().item():.3e})",
                        pytrace=False)


@pytest.mark.parametrize("history", list(REQUESTS))
def test_probe_requests_after_another_request_equal_a_fresh_pipeline(served, history):
    """The history request(s), then both probe requests, on the pipeline object every case of this module shares: the cases accumulate
    (engines grown by the long prompt and the eight regions stay grown, engines of another size stay cached)."""
    p, fresh = served
    on = REQUESTS[history](p)
    if on is not None:                                    # teeth: the option changed the rich probe while it was on
        assert not torch.equal(on, fresh[0][0]), f"{history}: the option changes no bit of the rich probe"
    _check(p, fresh, history)


def test_the_histories_again_in_reverse_order(served):
    p, fresh = served
    done = []
    for history in reversed(list(REQUESTS)):
        REQUESTS[history](p)
        done.append(history)
        _check(p, fresh, " -> ".join(done))


# ---------------------------------------------------------------------------------------------------------------- the serving path
def test_requests_file_order_does_not_change_a_requests_images(tmp_path):
    """`sample --requests FILE` on a tiny SD checkpoint directory with an IP-Adapter: five lines that differ in scheduler, FreeU, image
    prompts, prompt chunks and seed, run in file order, reversed, and as five one-line files.  Every request's two images are the same
    bytes in all three; the first and the last line are the same request and give the same bytes inside one run too."""
    from safetensors.torch import save_file
    from oracle.unet import TINY_SD_CONFIG, random_state_dict
    from rich_text_to_image_amd import sample
    from tests.test_checkpoint_gpu import _write_dir
    ckpt = str(tmp_path / "ckpt")
    _write_dir(ckpt)
    ck, _ = synthetic_checkpoint(TINY_SD_CONFIG, random_state_dict(TINY_SD_CONFIG, seed=1), T=4, E=24, seed=5)
    save_file({k: v.contiguous() for k, v in ck.items()}, str(tmp_path / "adapter.safetensors"))
    g = torch.Generator().manual_seed(13)
    for name in ("a.pt", "b.pt"):
        torch.save(torch.randn(24, generator=g), str(tmp_path / name))

    def rich(tail):
        return {"ops": [{"insert": "a "}, {"attributes": {"link": "a wooden fence covered in snow"}, "insert": "fence"}, {"insert": " and a "},
                        {"attributes": {"font": "slabo"}, "insert": "barn"}, {"insert": tail + "\n"}]}
    short, long_ = rich(" under a night sky"), rich(" under a night sky with bright stars and a pale moon above quiet hills far away in the cold")
    lines = [{"rich_text_json": short, "seed": 3},
             {"rich_text_json": short, "seed": 4, "scheduler": "sde-dpmsolver++", "freeu": [0.9, 0.2, 1.5, 1.6]},
             {"rich_text_json": short, "seed": 3, "image_prompts": [f"{tmp_path / 'a.pt'}:base:0.8", {"file": str(tmp_path / "b.pt"), "target": 0, "scale": -0.5}]},
             {"rich_text_json": long_, "seed": 5, "max_prompt_chunks": 3, "scheduler": "dpmsolver++"},
             {"rich_text_json": short, "seed": 3}]

    def run(name, order):
        f = tmp_path / f"{name}.jsonl"
        f.write_text("".join(json.dumps(lines[k]) + "\n" for k in order))
        out = tmp_path / name
        sample.main(["--load_path", ckpt, "--model", "SD", "--sample_steps", "12", "--num_segments", "4", "--inject_selfattn", "0.3",
                     "--ip_adapter", str(tmp_path / "adapter.safetensors"), "--requests", str(f), "--run_dir", str(out)])
        got = {}
        for pos, k in enumerate(order):
            tag = f"seed{lines[k]['seed']}" if len(order) == 1 else f"req{pos}_seed{lines[k]['seed']}"
            got[k] = tuple(open(out / f"{tag}_{kind}.jpg", "rb").read() for kind in ("plain", "rich"))
        return got
    listed = run("listed", [0, 1, 2, 3, 4])
    assert listed[4] == listed[0], "the same request at the head and at the tail of one file"
    assert len({listed[k][1] for k in range(4)}) == 4, "the four different requests must give four different rich images"
    backwards = run("reversed", [4, 3, 2, 1, 0])
    for k in range(5):
        for kind, a, b in zip(("plain", "rich"), listed[k], backwards[k]):
            assert a == b, f"request {k}: the {kind} image depends on the order of the file"
    for k in range(5):
        alone = run(f"alone{k}", [k])
        for kind, a, b in zip(("plain", "rich"), listed[k], alone[k]):
            assert a == b, f"request {k}: the {kind} image differs between the file of five and a file of its own"
