"""Perturbed-attention guidance without a GPU: the oracle with perturbed attention and how far it moves the tiny models, the fp64
restatements of the guidance and of the fold, and the host logic - layer specs, slot scales, command line, --requests, stream plan."""
import json
import types

import pytest
import torch

import controlnet_ref as CR
import pag_ref as R
from freeu_ref import FORWARD_BAR, forward_case, oracle_streams, rel_l2
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet

STEP_BAR = 3e-2


# ---------------------------------------------------------------------------------------------------------------- the oracle
def _base_pair(c, applied):
    """(T, P, u) of the base stream (font size on) of forward_case `c` on the CPU oracle."""
    def added(k):
        return {"text_embeds": c["pooled"][k:k + 1], "time_ids": c["tid"]} if c["xl"] else None
    fs = {"fontsize": {"word_pos": c["wp"], "font_size": c["fs"]}}
    o, op = OracleUNet(c["cfg"], c["sd"]), R.PagOracleUNet(c["cfg"], c["sd"], applied)
    with torch.no_grad():
        return (o.forward(c["lat"], c["t"], c["emb"][2:3], added(2), ctl=fs), op.forward(c["lat"], c["t"], c["emb"][2:3], added(2), ctl=fs),
                o.forward(c["lat"], c["t"], c["emb"][:1], added(0)))


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_all_layers_discriminate_and_an_empty_set_is_the_plain_oracle(which):
    """With every attn1 module applied the twin of the base stream is at least 10 x FORWARD_BAR from its partner (measured: tiny XL 0.281,
    tiny SD 0.469; `mid` alone moves tiny SD by 0.0083, below the forward bar - so the forward and step tests apply all layers and test
    `mid` for layer selection by bits).  With an empty applied set PagOracleUNet returns OracleUNet's bits."""
    c = forward_case(which)
    every = R.all_attn1(c["cfg"])
    T, P, u = _base_pair(c, every)
    d = rel_l2(P, T)
    print(f"tiny {which}: all attn1 applied: twin from partner {d:.3f}, |T - P| / |T - u| = {float((T - P).norm() / (T - u).norm()):.2f}")
    assert d >= 10 * FORWARD_BAR
    T0, P0, _ = _base_pair(c, ())
    assert torch.equal(T0, P0) and torch.equal(T0, T)


# ---------------------------------------------------------------------------------------------------------------- fp64 restatements
def test_three_term_formula_with_masks_and_the_fold():
    """guidance_ref is u + g (sum m T - u) + sum m sigma (T - P); folding T' = T + (sigma / g) (T - P) first and then applying the
    two-term guidance gives the same numbers to 1e-12."""
    g = torch.Generator().manual_seed(5)
    h, w, R_, gs = 6, 10, 3, 5.0
    u = torch.randn(1, 4, h, w, generator=g, dtype=torch.float64)
    T = [torch.randn(1, 4, h, w, generator=g, dtype=torch.float64) for _ in range(R_)]
    P = [torch.randn(1, 4, h, w, generator=g, dtype=torch.float64) for _ in range(R_)]
    masks = list(torch.softmax(torch.randn(R_, 1, 1, h, w, generator=g, dtype=torch.float64), 0).expand(R_, 1, 4, h, w))
    sig = [2.0, 0.0, 3.0]
    P[1] = None
    got = R.guidance_ref(u, T, P, masks, sig, gs)
    by_hand = u + gs * (sum(m * t for m, t in zip(masks, T)) - u)
    for r in (0, 2):
        by_hand = by_hand + masks[r] * sig[r] * (T[r] - P[r])
    assert float((got - by_hand).abs().max()) <= 1e-12
    folded = [t if s == 0.0 else R.fold_ref(t, p, s / gs) for t, p, s in zip(T, P, sig)]
    two_term = u + gs * (sum(m * t for m, t in zip(masks, folded)) - u)
    assert float((two_term - got).abs().max()) <= 1e-12
    assert float((R.guidance_ref(u, T, P, masks, [0.0] * 3, gs) - got).abs().max()) > 0.1      # ... and PAG is not a no-op


def test_fold_bar_admits_fp32_and_rejects_a_dropped_fold():
    g = torch.Generator().manual_seed(6)
    t, p = torch.randn(4096, generator=g), torch.randn(4096, generator=g)
    rho = torch.tensor(3.0 / 5.0, dtype=torch.float32).item()
    fp32 = t + torch.tensor(rho) * (t - p)                               # two or three fp32 roundings
    ref, bar = R.fold_ref(t, p, rho), R.fold_bar(t, p, rho)
    assert bool(((fp32.double() - ref).abs() <= 1.5 * bar).all())
    assert float(((t.double() - ref).abs() > bar).double().mean()) > 0.9


def test_oracle_step_with_pag_is_far_from_the_step_without():
    """The oracle's latent update of the injected first step of rich_case with sigma = (base 3.0, region 0 2.0, region 1 0) is at least
    10 x STEP_BAR from the update without PAG, in both latent streams (at guidance scale pag_ref.STEP_GS; at rich_case's own 5.0 the main
    stream measures 0.292, a hair below)."""
    c = CR.rich_case()
    sched, lat0, gs = c["sched"], c["lat"], R.STEP_GS
    t = sched.timesteps[0]
    o, op = OracleUNet(c["cfg"], c["sd"]), R.PagOracleUNet(c["cfg"], c["sd"], R.all_attn1(c["cfg"]))
    lat_in = sched.scale_model_input(lat0, t)
    tfd = {"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])}
    masks = [c["masks"][r:r + 1] for r in range(3)]

    def added_fn(k):
        k = k if k >= 0 else c["pooled"].shape[0] + k
        return {"text_embeds": c["pooled"][k:k + 1], "time_ids": c["tid"]}

    def update(sig):
        e, er = R.rich_step_pag(o, op, lat_in, lat_in.clone(), t, c["emb"], added_fn, masks, tfd, True, sig, gs)
        out = sched.step(torch.cat([e, er]).float(), t, torch.cat([lat0, lat0]))["prev_sample"]
        return [x - lat0 for x in torch.chunk(out, 2, dim=0)]
    on, off = update((0.0, 2.0, 0.0, 3.0)), update((0.0,) * 4)
    d = [rel_l2(a, b) for a, b in zip(off, on)]
    print(f"oracle step, PAG on against off: latent UPDATE rel-L2 {d[0]:.3f} (reference stream {d[1]:.3f})")
    assert min(d) >= 10 * STEP_BAR, d


# ---------------------------------------------------------------------------------------------------------------- host logic
def test_layer_specs_resolve_to_module_names():
    from rich_text_to_image_amd.engine import Engine
    from rich_text_to_image_amd.pag import DEFAULT_LAYERS, resolve_layers
    for cfg in (TINY_XL_CONFIG, TINY_SD_CONFIG):
        e = Engine(cfg, 8, 8, device=-1)
        try:
            mods = e.attn_modules()
        finally:
            e.close()
        a1 = [n for n, _, _ in mods if n.endswith(".attn1")]
        assert resolve_layers(("down", "mid", "up"), mods) == a1 == R.all_attn1(cfg)
        mid = resolve_layers(DEFAULT_LAYERS, mods)
        assert mid and all(n.startswith("mid_block.") for n in mid) and mid == resolve_layers("mid_block", mods) == resolve_layers("mid_block.attentions.0", mods)
        first_down = a1[0].split(".attentions.")[0]
        got = resolve_layers((first_down, "mid"), mods)
        assert got == [n for n in a1 if n.startswith(first_down + ".") or n.startswith("mid_block.")]      # execution order, each once
        assert resolve_layers((a1[-1], "up", a1[-1]), mods) == [n for n in a1 if n.startswith("up_blocks.")]
        one = resolve_layers(first_down + ".attentions.1", mods)
        assert one and all(n.startswith(first_down + ".attentions.1.") for n in one)
        for bad, word in (("bogus", "bogus"), ("down_blocks.9", "down_blocks.9"), (a1[0][:-1] + "2", "attn2"), ("", "non-empty"), ("mid.attentions.0", "mid.attentions.0")):
            with pytest.raises(ValueError) as ex:
                resolve_layers((bad,), mods)
            assert word in str(ex.value), (bad, str(ex.value))


def test_engine_refuses_bad_layer_names_by_name():
    """rt_set_pag_layers needs no device: an unknown name and an attn2 name are refused naming the offender; a good set is taken."""
    from rich_text_to_image_amd.engine import Engine, RtError
    e = Engine(TINY_XL_CONFIG, 8, 8, device=-1)
    try:
        a1 = R.all_attn1(TINY_XL_CONFIG)
        e.set_pag_layers(a1)
        e.set_pag_layers([])
        for bad, word in (("mid_block.attentions.0.transformer_blocks.7.attn1", "transformer_blocks.7.attn1"), (a1[0][:-1] + "2", "cross-attention")):
            with pytest.raises(RtError) as ex:
                e.set_pag_layers([a1[0], bad])
            assert ex.value.code == -1 and word in str(ex.value)
    finally:
        e.close()


def test_slot_scales_and_set_pag_checks():
    from rich_text_to_image_amd.pag import PagMixin, check_guidance, slot_scales, twin_count
    m = PagMixin()
    assert m.pag is None and m.pag_slot_scales(4, True) is None
    m.set_pag()
    assert m.pag == dict(scale=3.0, regions={}, base=None, layers=("mid",))
    assert m.pag_slot_scales(4, True) == [0.0, 3.0, 3.0, 3.0] and m.pag_slot_scales(2, False) == [0.0, 3.0]
    m.set_pag(scale=2.0, regions={1: 0.0}, base=3.0, layers="up")
    assert m.pag_slot_scales(4, True) == [0.0, 2.0, 0.0, 3.0]             # [negative, region 0, region 1, base]: the negative slot has no twin
    assert m.pag_slot_scales(2, False) == [0.0, 3.0]                      # the plain pass: regions are not read
    assert twin_count([0.0, 2.0, 0.0, 3.0], True) == 3 and twin_count([0.0, 3.0], False) == 1 and twin_count(None, True) == 0
    assert twin_count([0.0, 2.0, 0.0, 0.0], True) == 1
    with pytest.raises(ValueError) as ex:
        m.set_pag(regions={2: 1.0})
        m.pag_slot_scales(4, True)
    assert "region 2" in str(ex.value)
    for kw in (dict(scale=float("nan")), dict(scale="x"), dict(base=float("inf")), dict(regions={0: float("nan")}), dict(regions={-1: 1.0}),
               dict(regions={True: 1.0}), dict(regions=[1.0]), dict(layers=()), dict(layers=("",)), dict(scale=True)):
        with pytest.raises(ValueError):
            PagMixin().set_pag(**kw)
    m.set_pag(scale=3.0)
    for g, phi, word in ((0.0, 0.0, "guidance_scale"), (5.0, 0.5, "guidance_rescale")):
        with pytest.raises(ValueError) as ex:
            m.pag_slot_scales(4, True, g, phi)
        assert word in str(ex.value)
    check_guidance([0.0, 0.0], 0.0, 0.5)                                  # every sigma 0: PAG is off, nothing is refused
    m.clear_pag()
    assert m.pag is None


def test_command_line_and_requests_forms(tmp_path):
    from rich_text_to_image_amd.pag import pag_from_request, parse_scale_args
    from rich_text_to_image_amd.sample import build_parser, build_requests, check_pag_args
    assert parse_scale_args(["3"]) == dict(scale=3.0, regions={}, base=None)
    assert parse_scale_args(["2", "1:0", "base:3.5"]) == dict(scale=2.0, regions={1: 0.0}, base=3.5)
    assert parse_scale_args(["0:4"]) == dict(scale=0.0, regions={0: 4.0}, base=None)      # only region 0: everything else off
    for bad in (["x"], ["negative:1"], ["1:nan"], ["2", "3"], ["base:1", "base:2"], ["1:1", "1:2"], ["1:"]):
        with pytest.raises(ValueError):
            parse_scale_args(bad)
    assert pag_from_request(3) == dict(scale=3.0, regions={}, base=None, layers=("mid",))
    assert pag_from_request({"scale": [2, "0:1"], "layers": ["up", "mid"]}) == dict(scale=2.0, regions={0: 1.0}, base=None, layers=("up", "mid"))
    for bad in ({"scale": 3, "window": 1}, {"layers": []}, None, True, {"scale": "x"}):
        with pytest.raises(ValueError):
            pag_from_request(bad)
    j = '{"ops":[{"insert":"a cat\\n"}]}'
    a = build_parser().parse_args(["--rich_text_json", j, "--pag_scale", "3", "1:0", "--pag_layers", "mid", "up_blocks.0"])
    a.pag = check_pag_args(a)
    assert a.pag == dict(scale=3.0, regions={1: 0.0}, base=None, layers=("mid", "up_blocks.0"))
    assert build_requests(a)[0]["pag"] == a.pag
    assert build_requests(build_parser().parse_args(["--rich_text_json", j]))[0]["pag"] is None
    f = tmp_path / "reqs.jsonl"
    f.write_text(json.dumps({"rich_text_json": json.loads(j), "pag": {"scale": [1.5, "base:2"], "layers": ["down"]}}) + "\n" + json.dumps({"rich_text_json": json.loads(j)}) + "\n")
    ns = types.SimpleNamespace(requests=str(f), rich_text_json=None, seeds=None, seed=6, negative_prompt="", freeu=None, pag=a.pag)
    r = build_requests(ns)
    assert r[0]["pag"] == dict(scale=1.5, regions={}, base=2.0, layers=("down",)) and r[1]["pag"] == a.pag      # a line's own, else the flags'


def test_generate_sets_the_request_and_restores_it(monkeypatch):
    """param['pag'] is the pipeline attribute for the duration of the request - also when the request fails - and the earlier request
    comes back after it: it does not leak into the next request."""
    from rich_text_to_image_amd import sample
    from rich_text_to_image_amd.pag import PagMixin
    seen = []

    def body(model, param, *a):
        seen.append((model.pag, "pag" in param))
        if param.get("boom"):
            raise RuntimeError("boom")
        return "plain", "rich", {}
    monkeypatch.setattr(sample, "_generate", body)
    m = PagMixin()
    sample.generate(m, {"pag": dict(scale=2.0, regions={0: 1.0}, base=None, layers=("mid",))})
    assert seen[-1] == (dict(scale=2.0, regions={0: 1.0}, base=None, layers=("mid",)), False) and m.pag is None
    sample.generate(m, {"pag": None})
    assert seen[-1][0] is None
    m.set_pag(scale=1.0)
    keep = dict(m.pag)
    with pytest.raises(RuntimeError):
        sample.generate(m, {"pag": dict(scale=4.0, regions={}, base=None, layers=("up",)), "boom": True})
    assert seen[-1][0]["scale"] == 4.0 and m.pag == keep
    with pytest.raises(ValueError):
        sample.generate(m, {"pag": dict(scale=float("nan"))})
    assert m.pag == keep


@pytest.mark.parametrize("argv", [["--pag_scale", "x"], ["--pag_scale", "negative:1"], ["--pag_layers", "mid"], ["--pag_scale", "3", "--pag_layers", "bogus"],
                                  ["--pag_scale", "3", "--guidance_rescale", "0.5"], ["--pag_scale", "3", "--guidance_weight", "0"], ["--requests", "BAD"],
                                  ["--requests", "RESCALE"]])
def test_bad_values_and_refused_combinations_end_the_run_before_any_rank_starts(argv, tmp_path, monkeypatch):
    from rich_text_to_image_amd import launcher, sample

    def never(*a, **k):
        raise AssertionError("the launch was reached")
    monkeypatch.setattr(launcher, "self_launch", never)
    monkeypatch.setattr(launcher, "init_distributed", never)
    j = '{"ops":[{"insert":"a cat\\n"}]}'
    if argv[0] == "--requests":
        f = tmp_path / "reqs.jsonl"
        bad = {"scale": ["1", "nope:2"]} if argv[1] == "BAD" else 3.0
        f.write_text(json.dumps({"rich_text_json": json.loads(j)}) + "\n" + json.dumps({"rich_text_json": json.loads(j), "pag": bad}) + "\n")
        argv = ["--requests", str(f)] + (["--guidance_rescale", "0.5"] if argv[1] == "RESCALE" else [])
    with pytest.raises(SystemExit) as e:
        sample.main(["--rich_text_json", j, "--gpus", "2"] + argv)
    msg = str(e.value.code)                                              # check_pag_args' own refusal, not argparse's (whose code is 2)
    assert msg.startswith("sample: ") and ("pag" in msg), msg


def test_full_module_names_with_any_block_index_pass_the_precheck():
    """Before the UNet is known only the FORM of a layer spec is checked: a full attn1 name with transformer_blocks.K, K > 0 (SDXL has up to
    10 per attention), passes; an attn2 name and a malformed one do not."""
    from rich_text_to_image_amd.pag import check_layer_forms
    from rich_text_to_image_amd.sample import build_parser, check_pag_args
    j = '{"ops":[{"insert":"a cat\\n"}]}'
    names = ["mid_block.attentions.0.transformer_blocks.5.attn1", "down_blocks.2.attentions.1.transformer_blocks.9.attn1", "up_blocks.0.attentions.2.transformer_blocks.0.attn1"]
    a = build_parser().parse_args(["--rich_text_json", j, "--pag_scale", "3", "--pag_layers"] + names + ["mid", "up_blocks.1", "down_blocks.2.attentions.0"])
    assert check_pag_args(a)["layers"] == tuple(names) + ("mid", "up_blocks.1", "down_blocks.2.attentions.0")
    for bad, word in (("mid_block.attentions.0.transformer_blocks.5.attn2", "cross-attention"), ("mid_block.attentions.0.transformer_blocks.x.attn1", "unknown"),
                      ("mid_block.transformer_blocks.0.attn1", "unknown"), ("", "non-empty")):
        with pytest.raises(ValueError) as ex:
            check_layer_forms([bad])
        assert word in str(ex.value)
        if bad:
            with pytest.raises(SystemExit) as e:
                check_pag_args(build_parser().parse_args(["--rich_text_json", j, "--pag_scale", "3", "--pag_layers", bad]))
            assert word in str(e.value.code)


def test_stream_plan_lists():
    """The stream list of a rich step with R = 3 as csrc/step_driver.inl::region_plan builds it (restated by pag.expected_streams; the GPU
    test compares the engine's count): twins behind all existing streams - base, text_ref only while the pair is stepped, then the
    regions with sigma != 0."""
    from rich_text_to_image_amd.pag import expected_streams
    sig = [0.0, 2.0, 0.0, 3.0]
    head = ["uncond", "base", "uncond_ref", "text_ref"]
    assert expected_streams(3, sig, True, True) == head + ["region0<-text_ref", "region1<-text_ref", "twin(base)", "twin(text_ref)", "twin(region0)"]
    assert expected_streams(3, sig, False, True) == head + ["region0", "region1", "twin(base)", "twin(text_ref)", "twin(region0)"]
    assert expected_streams(3, sig, False, False) == head + ["region0", "region1", "twin(base)", "twin(region0)"]      # the pair runs but is not stepped
    assert expected_streams(3, sig, False, False, run_ref=False) == ["uncond", "base", "region0", "region1", "twin(base)", "twin(region0)"]      # elided pair
    assert expected_streams(3, [0.0, 2.0, 1.0, 0.0], True, True) == head + ["region0<-text_ref", "region1<-text_ref", "twin(region0)", "twin(region1)"]
    assert expected_streams(3, [0.0] * 4, True, True) == expected_streams(3, None, True, True) == head + ["region0<-text_ref", "region1<-text_ref"]


def test_plain_split_ranges_follow_the_stream_count():
    """launcher.split_plain_step's ranges with and without the twin: it rides with the text stream's part."""
    from rich_text_to_image_amd import launcher
    calls = []

    class Eng:
        def __init__(self, n):
            self.n = n

        def plain_streams(self):
            return self.n

        def plain_step(self, i, g):
            calls.append(("whole", i))
    assert launcher.split_plain_step(Eng(3), 0, 5.0) == [(0, 3)] and calls == [("whole", 0)]      # one rank: the engine's own step
    assert launcher.split_plain_step(Eng(2), 1, 5.0) == [(0, 2)]
    # the rule itself, for every world size: the ranges are contiguous, cover every stream once and keep the twin with the text stream
    assert launcher.plain_ranges(2, 2) == [(0, 1), (1, 1)] and launcher.plain_ranges(3, 2) == [(0, 1), (1, 2)]
    assert launcher.plain_ranges(2, 4) == [(0, 1), (1, 1), (2, 0), (2, 0)] and launcher.plain_ranges(3, 4) == [(0, 1), (1, 2), (3, 0), (3, 0)]
    assert launcher.plain_ranges(3, 1) == [(0, 3)]


def test_split_plain_step_follows_the_engine_ranges_on_two_ranks(monkeypatch):
    """launcher.split_plain_step on a faked process group of two: each rank's own range from the engine equals the rule's, the twin's
    prediction travels with the text stream's broadcast, and every rank finishes."""
    from rich_text_to_image_amd import launcher
    sent = []

    class Eng:
        device = 0

        def __init__(self, rank):
            self.rank, self.done = rank, False

        def plain_streams(self):
            return 3

        def plain_step_part(self, i, part, nparts):                      # csrc/step_driver.inl::plain_step_part with a twin
            return (0, 1) if part == 0 else (1, 2) if part == 1 else (3, 0)

        def synchronize(self):
            pass

        def eps_as_tensor(self):
            return torch.zeros(3 * 8), 8

        def plain_step_finish(self, i, g):
            self.done = True
    monkeypatch.setattr(launcher.dist, "is_initialized", lambda: True)
    monkeypatch.setattr(launcher.dist, "get_world_size", lambda: 2)
    monkeypatch.setattr(launcher, "broadcast_tensor", lambda t, src: sent.append((src, t.numel())))
    monkeypatch.setattr(launcher, "_cuda_sync", lambda: None)
    for rank in (0, 1):
        monkeypatch.setattr(launcher.dist, "get_rank", lambda r=rank: r)
        e = Eng(rank)
        del sent[:]
        assert launcher.split_plain_step(e, 0, 5.0) == [(0, 1), (1, 2)] and e.done
        assert sent == [(0, 8), (1, 16)]
