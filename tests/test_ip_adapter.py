"""Image prompts without a GPU: the op bar of tests/ip_adapter_ref.py against a CPU emulation of an honest kernel and of three faulty
ones, the oracle hook against the plain oracle and a direct restatement of diffusers' processor, the checkpoint loader, the facade and
command-line validation, and the weight table of an engine built with image tokens."""
import json
import math

import pytest
import torch

import ip_adapter_ref as R
from oracle.shapes import weight_shapes
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict

CONFIGS = {"xl": TINY_XL_CONFIG, "sd": TINY_SD_CONFIG}


# ---------------------------------------------------------------------------------------------------------------- the bar
@pytest.mark.parametrize("N,H,d,DP,T", R.OP_CASES, ids=[f"N{c[0]}-H{c[1]}-d{c[2]}to{c[3]}-T{c[4]}" for c in R.OP_CASES])
def test_the_bar_passes_an_honest_kernel_and_catches_faulty_ones(N, H, d, DP, T):
    """On the inputs of the GPU op test: the emulation of an honest kernel (fp32 scores, exp2, P to bf16, fp32 PV, one rounding) stays
    within the bar on every element; a scale 2 % off, one pad key scored instead of masked (where the slot has one) and a missing image
    term each put at least 15 % of the elements of the real columns over it."""
    Q, K, V, O = R.op_inputs(N, H, d, DP, T)
    counts = [T, 1, T]
    ref, bar = R.op_ref(Q, K, V, O, R.OP_SLOTS, counts, R.OP_SCALES)

    def stat(x):
        return R.worst_and_share(x[..., :d], ref[..., :d], bar[..., :d])
    worst, share = stat(R.emulate(Q, K, V, O, R.OP_SLOTS, counts, R.OP_SCALES))
    print(f"honest kernel: worst {worst:.3f}")
    assert worst <= 1.0 and share == 0.0
    faulty = {"scale 2 % off": dict(scale_err=1.02), "image term missing": dict(drop_term=True)}
    if T < 16:
        faulty["one pad key unmasked"] = dict(extra_keys=1)
    for name, kw in faulty.items():
        worst, share = stat(R.emulate(Q, K, V, O, R.OP_SLOTS, counts, R.OP_SCALES, **kw))
        print(f"{name}: worst {worst:.1f}, share over the bar {share:.3f}")
        assert share >= 0.15, name
    # the skipped entry and the pad columns carry no bar and no change
    assert torch.equal(ref[1], O[1].double()) and float(bar[1].max()) == 0.0
    assert torch.equal(ref[..., d:], O[..., d:].double())


# ---------------------------------------------------------------------------------------------------------------- the oracle hook
def _small_forward(which):
    cfg = CONFIGS[which]
    sd = random_state_dict(cfg, seed=3)
    g = torch.Generator().manual_seed(5)
    lat = torch.randn(2, 4, 16, 16, generator=g)
    emb = torch.randn(2, 77, cfg["cross_attention_dim"], generator=g)
    added = {"text_embeds": torch.randn(2, 32, generator=g), "time_ids": torch.tensor([[128.0, 128.0, 0, 0, 128.0, 128.0]] * 2)} if which == "xl" else None
    return cfg, sd, lat, emb, added


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_hook_with_scale_0_is_the_plain_oracle_bit_for_bit(which):
    cfg, sd, lat, emb, added = _small_forward(which)
    sd_ip = dict(sd); sd_ip.update(R.ip_weights(sd, 5))
    tk = torch.randn(4, cfg["cross_attention_dim"], generator=torch.Generator().manual_seed(1))
    with torch.no_grad():
        want = OracleUNet(cfg, sd).forward(lat, 500.0, emb, added)
        o = OracleUNet(cfg, sd_ip)
        o.attn_impl = R.ip_attn_impl([tk, None], [0.0, 1.0])
        assert torch.equal(o.forward(lat, 500.0, emb, added), want)
        o.attn_impl = R.ip_attn_impl([tk, None], [1.0, 0.0])                # per batch entry: entry 1 keeps its bits, entry 0 moves
        got = o.forward(lat, 500.0, emb, added)
    assert torch.equal(got[1], want[1]) and not torch.equal(got[0], want[0])


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_hook_with_one_global_image_is_diffusers_processor(which):
    """One image for every batch entry: the hook equals a direct restatement of diffusers' IPAdapterAttnProcessor to 1e-12 in fp64."""
    cfg = CONFIGS[which]
    sd = random_state_dict(cfg, seed=3)
    sd.update(R.ip_weights(sd, 5))
    o = OracleUNet(cfg, sd)
    o.sd = {k: v.double() for k, v in sd.items()}
    g = torch.Generator().manual_seed(8)
    from rich_text_to_image_amd.ip_adapter import attn2_names
    for name, C in attn2_names(cfg)[::3]:
        nh = _heads(cfg, name)
        x = torch.randn(2, 24, C, generator=g, dtype=torch.float64)
        text = torch.randn(2, 77, cfg["cross_attention_dim"], generator=g, dtype=torch.float64)
        tk = torch.randn(5, cfg["cross_attention_dim"], generator=g, dtype=torch.float64)
        got, _ = R.ip_attn_impl([tk, tk], [0.7, 0.7])(o, name, x, nh, text, None, None)
        want = R.diffusers_processor(o.sd, name, nh, x, text, tk[None].expand(2, -1, -1), 0.7)
        assert (got - want).abs().max().item() <= 1e-12 * max(1.0, want.abs().max().item()), name
        plain, _ = o._attention(name, x, nh, ctx=text)
        assert (got - plain).abs().max().item() > 1e-3


def _heads(cfg, name):
    n = len(cfg["block_out_channels"])
    heads = cfg["attention_head_dim"] if isinstance(cfg["attention_head_dim"], (tuple, list)) else (cfg["attention_head_dim"],) * n
    p = name.split(".")
    if p[0] == "down_blocks":
        return heads[int(p[1])]
    if p[0] == "up_blocks":
        return heads[n - 1 - int(p[1])]
    return heads[-1]


# ---------------------------------------------------------------------------------------------------------------- the loader
@pytest.mark.parametrize("which", ["xl", "sd"])
@pytest.mark.parametrize("layout", ["original", "nested", "diffusers"])
def test_loader_reads_both_layouts_in_the_processor_order(which, layout, tmp_path):
    from rich_text_to_image_amd.ip_adapter import attn2_names, load_ip_adapter
    cfg = CONFIGS[which]
    sd = random_state_dict(cfg, seed=3)
    ck, want = R.synthetic_checkpoint(cfg, sd, T=4, E=24, layout=layout)
    ad = load_ip_adapter(ck, cfg)
    assert ad["T"] == 4 and ad["D"] == cfg["cross_attention_dim"] and ad["E"] == 24
    assert set(ad["weights"]) == set(want) and all(torch.equal(ad["weights"][k], want[k]) for k in want)
    assert set(ad["image_proj"]) == {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}
    # the order: down blocks, then up blocks, then the mid block - and the same list as the test's own restatement
    names = [n for n, _ in attn2_names(cfg)]
    assert names == R.attn2_names(cfg)
    kinds = [n.split(".")[0] for n in names]
    assert kinds == sorted(kinds, key=("down_blocks", "up_blocks", "mid_block").index) and kinds[-1] == "mid_block"
    assert set(n + ".to_k.weight" for n in names) == {k for k in sd if k.endswith(".attn2.to_k.weight")}
    if layout == "original":                                         # ip_adapter.{2 k + 1} = the k-th attn2: swapping two layers is seen
        assert torch.equal(ad["weights"][names[1] + ".to_v_ip.weight"], ck["ip_adapter.3.to_v_ip.weight"])
        from safetensors.torch import save_file
        f = str(tmp_path / "ip.safetensors")
        save_file({k: v.contiguous() for k, v in ck.items()}, f)
        ad2 = load_ip_adapter(f, cfg)
        assert all(torch.equal(ad2["weights"][k], want[k]) for k in want)
        b = str(tmp_path / "ip.bin")
        torch.save(ck, b)
        assert load_ip_adapter(b, cfg)["T"] == 4
    # T from proj's rows
    ck16, _ = R.synthetic_checkpoint(cfg, sd, T=16, E=8, layout=layout)
    assert load_ip_adapter(ck16, cfg)["T"] == 16


def test_loader_errors_name_the_key():
    from rich_text_to_image_amd.ip_adapter import load_ip_adapter
    cfg = TINY_XL_CONFIG
    sd = random_state_dict(cfg, seed=3)
    ck, _ = R.synthetic_checkpoint(cfg, sd)

    def broken(f):
        c = dict(ck)
        f(c)
        return c
    D = cfg["cross_attention_dim"]
    cases = [
        (lambda c: c.pop("ip_adapter.5.to_v_ip.weight"), "ip_adapter.5.to_v_ip.weight"),
        (lambda c: c.pop("image_proj.norm.bias"), "image_proj.norm.bias"),
        (lambda c: c.update({"ip_adapter.99.to_k_ip.weight": torch.zeros(8, D)}), "ip_adapter.99.to_k_ip.weight"),
        (lambda c: c.update({"ip_adapter.1.to_k_ip.weight": torch.zeros(7, D)}), "ip_adapter.1.to_k_ip.weight"),
        (lambda c: c.update({"image_proj.latents": torch.zeros(1, 16, 8)}), "Resampler"),
        (lambda c: c.update({"image_proj.proj.weight": torch.zeros(17 * D, 24)}), "image_proj.proj.weight"),
        (lambda c: c.update({"image_proj.proj.weight": torch.zeros(4 * D + 1, 24)}), "image_proj.proj.weight"),
        (lambda c: c.update({"image_proj.norm.weight": torch.zeros(D + 1)}), "image_proj.norm.weight"),
    ]
    for f, word in cases:
        with pytest.raises(ValueError) as e:
            load_ip_adapter(broken(f), cfg)
        assert word in str(e.value), (word, str(e.value))
    with pytest.raises(ValueError) as e:                             # an SD adapter on the XL UNet
        load_ip_adapter(R.synthetic_checkpoint(TINY_SD_CONFIG, random_state_dict(TINY_SD_CONFIG, seed=3))[0], cfg)
    assert "image_proj." in str(e.value) or "ip_adapter." in str(e.value)
    with pytest.raises(ValueError):
        load_ip_adapter("/nonexistent/ip.safetensors", cfg)


def test_projection_restatement_shapes():
    cfg = TINY_SD_CONFIG
    ck, _ = R.synthetic_checkpoint(cfg, random_state_dict(cfg, seed=3), T=4, E=24, layout="nested")
    t = R.project_ref(ck["image_proj"], torch.randn(24))
    assert t.shape == (4, cfg["cross_attention_dim"]) and bool(torch.isfinite(t).all())
    assert (t.mean(-1).abs() < 0.2).all()                            # LayerNorm with weights near 1 and biases near 0


# ---------------------------------------------------------------------------------------------------------------- facade / command line
def _pipeline(which="xl"):
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    cfg = CONFIGS[which]
    sd = random_state_dict(cfg, seed=3)
    m = RegionDiffusionXL(device=0, unet_state_dict=sd, config=cfg) if which == "xl" else RegionDiffusion(0, unet_state_dict=sd, config=cfg)
    return m, cfg, sd


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_facade_validation(which):
    m, cfg, sd = _pipeline(which)
    D = cfg["cross_attention_dim"]
    with pytest.raises(ValueError):                                  # no adapter yet
        m.set_image_prompts(base=dict(embeds=torch.zeros(24)))
    ck, _ = R.synthetic_checkpoint(cfg, sd, T=4, E=24)
    m.load_ip_adapter(ck)
    assert m.unet.ip_tokens == 4 and m.image_prompts is None
    for bad in (dict(base=dict(embeds=torch.zeros(23))), dict(base=dict(tokens=torch.zeros(5, D))), dict(base=dict(tokens=torch.zeros(4, D + 1))),
                dict(base=dict(embeds=torch.zeros(24), tokens=torch.zeros(4, D))), dict(base=dict(scale=1.0)), dict(base=dict(embeds=torch.zeros(24), scale=float("nan"))),
                dict(base=dict(embeds=torch.zeros(24), weight=2.0)), dict(regions=[dict(embeds=torch.zeros(24))]), dict(regions={-1: dict(embeds=torch.zeros(24))}),
                dict(regions={"0": dict(embeds=torch.zeros(24))}), dict(negative=dict(embeds=torch.full((24,), float("inf")))), dict(base="image.png")):
        with pytest.raises(ValueError):
            m.set_image_prompts(**bad)
        assert m.image_prompts is None
    m.set_image_prompts(base=dict(embeds=torch.ones(24), scale=0.5), regions={1: dict(tokens=torch.ones(3, D))})
    # slots of a rich request [negative, region 0, region 1, base] and of the plain pass [negative, base]
    s = m.image_prompt_slots(4, True)
    assert sorted(s) == [2, 3] and s[3]["scale"] == 0.5 and s[2]["scale"] == 1.0 and s[2]["tokens"].shape == (3, D)
    assert sorted(m.image_prompt_slots(2, False)) == [1]
    with pytest.raises(ValueError) as e:                             # region 1 of a request with one region: before any launch
        m.image_prompt_slots(3, True)
    assert "region 1" in str(e.value)
    m.set_image_prompts(negative=dict(embeds=torch.zeros(24)))
    assert sorted(m.image_prompt_slots(4, True)) == [0]
    m.clear_image_prompts()
    assert m.image_prompts is None and m.image_prompt_slots(4, True) is None
    m.set_image_prompts(base=dict(embeds=torch.ones(24)))
    m.unload_ip_adapter()
    assert m.unet.ip_tokens == 0 and m.ip_adapter is None and m.image_prompts is None


def test_unet_object_takes_the_adapter_too():
    from rich_text_to_image_amd.unet import HipUNet2DConditionModel
    cfg = TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=3)
    u = HipUNet2DConditionModel(cfg, sd)
    ck, want = R.synthetic_checkpoint(cfg, sd, T=8, E=24, layout="diffusers")
    u.load_ip_adapter(ck)
    assert u.ip_tokens == 8 and set(u._ip_weights) == set(want)
    u.unload_ip_adapter()
    assert u.ip_tokens == 0 and u._ip_weights is None


def test_command_line_validation(tmp_path):
    from rich_text_to_image_amd import sample
    from rich_text_to_image_amd.ip_adapter import image_prompts_from_specs, parse_embeds_arg
    assert parse_embeds_arg("a.pt") == ("a.pt", "base", 1.0)
    assert parse_embeds_arg("a.npy:negative") == ("a.npy", "negative", 1.0)
    assert parse_embeds_arg("dir/a.safetensors:2:0.35") == ("dir/a.safetensors", 2, 0.35)
    assert parse_embeds_arg("a.pt::0.5") == ("a.pt", "base", 0.5)
    for bad in ("a.pt:left", "a.pt:1:much", "a.pt:1:nan", "a.pt:1:2:3", ":base", "a.png", "a.pt:-1"):
        with pytest.raises(ValueError):
            parse_embeds_arg(bad)
    ip = image_prompts_from_specs(["a.pt", "b.pt:0:0.5", {"file": "c.npy", "target": "negative"}])
    assert ip["base"] == dict(file="a.pt", scale=1.0) and ip["regions"] == {0: dict(file="b.pt", scale=0.5)} and ip["negative"]["file"] == "c.npy"
    with pytest.raises(ValueError):
        image_prompts_from_specs(["a.pt", "b.pt:base"])             # two prompts for one target
    # main(): bad values end the run before any rank starts
    emb, ad = tmp_path / "e.pt", tmp_path / "ip.bin"
    torch.save(torch.zeros(24), emb)
    torch.save({}, ad)
    js = json.dumps({"ops": [{"insert": "a cat\n"}]})
    base = ["--rich_text_json", js, "--gpus", "2", "--dry_launch"]
    for argv, word in ((["--ip_image_embeds", str(emb)], "needs --ip_adapter"),
                       (["--ip_adapter", str(tmp_path / "none.bin")], "file not found"),
                       (["--ip_adapter", str(ad), "--ip_image_embeds", str(tmp_path / "none.pt")], "file not found"),
                       (["--ip_adapter", str(ad), "--ip_image_embeds", f"{emb}:sky"], "TARGET"),
                       (["--ip_adapter", str(ad), "--ip_image_embeds", f"{emb}:0:inf"], "SCALE")):
        with pytest.raises(SystemExit) as e:
            sample.main(base + argv)
        assert word in str(e.value), (argv, str(e.value))
    req = tmp_path / "r.jsonl"
    req.write_text(json.dumps({"rich_text_json": {"ops": [{"insert": "a cat\n"}]}, "image_prompts": [f"{emb}:1:0.5", f"{emb}:oops"]}) + "\n")
    with pytest.raises(SystemExit) as e:
        sample.main(["--requests", str(req), "--ip_adapter", str(ad), "--gpus", "2", "--dry_launch"])
    assert "line 1" in str(e.value) and "TARGET" in str(e.value)
    # a good line: the request carries its own image prompts, the next one the flag's
    req.write_text(json.dumps({"rich_text_json": {"ops": [{"insert": "a cat\n"}]}, "image_prompts": [f"{emb}:1:0.5"]}) + "\n" +
                   json.dumps({"rich_text_json": {"ops": [{"insert": "a dog\n"}]}}) + "\n")
    a = sample.build_parser().parse_args(["--requests", str(req), "--ip_adapter", str(ad), "--ip_image_embeds", f"{emb}:base:0.25"])
    a.freeu = None
    a.image_prompts = sample.check_ip_args(a)
    reqs = sample.build_requests(a)
    assert reqs[0]["image_prompts"]["regions"] == {1: dict(file=str(emb), scale=0.5)} and reqs[0]["image_prompts"]["base"] is None
    assert reqs[1]["image_prompts"]["base"] == dict(file=str(emb), scale=0.25)


def test_generate_sets_the_requests_image_prompts_and_restores_the_pipelines(tmp_path, monkeypatch):
    from rich_text_to_image_amd import sample
    m, cfg, sd = _pipeline("xl")
    m.load_ip_adapter(R.synthetic_checkpoint(cfg, sd, T=4, E=24)[0])
    m.set_image_prompts(negative=dict(embeds=torch.ones(24)))
    keep = m.image_prompts
    f = tmp_path / "e.npy"
    import numpy as np
    np.save(f, np.ones((1, 24), dtype=np.float32))
    tk = tmp_path / "t.pt"
    torch.save(torch.ones(3, cfg["cross_attention_dim"]), tk)
    seen = {}
    monkeypatch.setattr(sample, "_generate", lambda model, param, *a: seen.update(ip=model.image_prompts, param=param) or "done")
    from rich_text_to_image_amd.ip_adapter import image_prompts_from_specs
    out = sample.generate(m, {"image_prompts": image_prompts_from_specs([f"{f}:base:0.5", f"{tk}:0"])}, "SDXL", str(tmp_path), 0.5, 0.0, 0.3, 9, 0.0)
    assert out == "done" and "image_prompts" not in seen["param"]
    assert seen["ip"]["base"]["scale"] == 0.5 and seen["ip"]["base"]["embeds"].shape == (24,) and seen["ip"]["regions"][0]["tokens"].shape == (3, cfg["cross_attention_dim"])
    assert m.image_prompts is keep


# ---------------------------------------------------------------------------------------------------------------- the weight table
@pytest.mark.parametrize("which", ["xl", "sd"])
def test_weight_table_with_image_tokens_is_the_reference_layout_plus_two_names_per_attn2(which):
    from rich_text_to_image_amd.engine import Engine, config_from_dict
    cfg = CONFIGS[which]
    ref = {k: tuple(v) for k, v in weight_shapes(cfg).items()}
    assert config_from_dict(cfg, 16, 16).ip_tokens == 0
    e0 = Engine(cfg, 16, 16, device=-1)
    e4 = Engine(cfg, 16, 16, device=-1, ip_tokens=4)
    try:
        t0, t4 = e0.weight_table(), e4.weight_table()
        assert dict(t0) == ref and len(t0) == len(ref)
        extra = {k: s for k, s in t4 if k not in ref}
        assert {k: s for k, s in t4 if k in ref} == ref and len(t4) == len(ref) + len(extra)
        names = R.attn2_names(cfg)
        D = cfg["cross_attention_dim"]
        assert extra == {f"{n}.{w}.weight": ref[f"{n}.to_k.weight"] for n in names for w in ("to_k_ip", "to_v_ip")}
        assert all(s[1] == D for s in extra.values()) and len(extra) == 2 * len(names)
    finally:
        e0.close(); e4.close()
    from rich_text_to_image_amd.engine import RtError
    for bad in (-1, 17):
        with pytest.raises(RtError):
            Engine(cfg, 16, 16, device=-1, ip_tokens=bad)


def test_a_broadcast_fed_model_refuses_an_adapter_once_it_has_an_engine():
    """A model built "empty" holds its weights in its engines' arena only: install_ip_adapter would drop them.  Before the first engine
    the adapter installs; afterwards load / unload raise and change nothing."""
    from rich_text_to_image_amd.unet import HipUNet2DConditionModel
    cfg = TINY_SD_CONFIG
    ck, _ = R.synthetic_checkpoint(cfg, random_state_dict(cfg, seed=3), T=8, E=24)
    u = HipUNet2DConditionModel(cfg, "empty")
    u.load_ip_adapter(ck)
    assert u.ip_tokens == 8
    u.unload_ip_adapter()

    class Held:
        closed = False

        def close(self):
            self.closed = True
    held = Held()
    u._engines[(16, 16)] = held
    with pytest.raises(RuntimeError):
        u.load_ip_adapter(ck)
    assert u.ip_tokens == 0 and u.ip_adapter is None and not held.closed and u._engines[(16, 16)] is held
    u2 = HipUNet2DConditionModel(cfg, "empty")
    u2.load_ip_adapter(ck)
    u2._engines[(16, 16)] = held
    with pytest.raises(RuntimeError):
        u2.unload_ip_adapter()
    assert u2.ip_tokens == 8 and u2.ip_adapter is not None and not held.closed
    u2._engines.clear()


def test_request_image_prompts_without_an_adapter_are_a_value_error(tmp_path):
    from rich_text_to_image_amd import sample
    from rich_text_to_image_amd.ip_adapter import image_prompts_from_specs
    m, cfg, sd = _pipeline("sd")
    f = tmp_path / "e.pt"
    torch.save(torch.ones(24), f)
    with pytest.raises(ValueError) as e:
        sample.generate(m, {"image_prompts": image_prompts_from_specs([str(f)])}, "SD", str(tmp_path), 0.5, 0.0, 0.3, 9, 0.0)
    assert "IP-Adapter" in str(e.value) and m.image_prompts is None
