"""Regional LoRA on the feed-forward, proj_in and proj_out without a GPU: the wider target set of regional_lora.parse_adapter, the weight
table of an engine with lora_targets, the bar of tests/regional_lora_ff_ref.py (an honest kernel's emulation passes, seven faulty ones do
not, the accumulation allowance is the measured one), and that the end-to-end cases of the GPU tests tell a forward with the four
modules from one without."""
import pytest
import torch

import regional_lora_ff_ref as F
import regional_lora_ref as R
from freeu_ref import FORWARD_BAR, forward_case, rel_l2
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict
from rich_text_to_image_amd import regional_lora as RL


@pytest.fixture(scope="module", params=["sd", "xl"])
def sd(request):
    return random_state_dict(TINY_XL_CONFIG if request.param == "xl" else TINY_SD_CONFIG, seed=11)


def _checkpoint(sd, layout, extra):
    """synthetic_adapter on the attention projections and `extra`; the diffusers 0.18 layout names attention processors only, so its
    further modules carry the names of its successor."""
    if layout != "diffusers018":
        return R.synthetic_adapter(sd, rank=4, seed=3, layout=layout, extra=extra)
    ck, truth = R.synthetic_adapter(sd, rank=4, seed=3, layout=layout)
    more, truth = R.synthetic_adapter(sd, rank=4, seed=3, layout="diffusers", extra=extra)
    ck.update({k: v for k, v in more.items() if any(k.startswith(f"unet.{p}.") for p in extra)})
    return ck, truth


def test_the_four_key_layouts_resolve_the_four_modules(sd):
    """linear (XL) and 1x1-convolution (SD) proj_in / proj_out alike: the factors arrive 2-D."""
    wide = F.wide_modules(sd)
    blocks = len(R.attention_projections(sd)) // 8
    assert len(wide) == 2 * blocks + 2 * len([p for p in wide if p.endswith(".proj_in")]) and len({p.rsplit(".", 1)[-1] for p in wide}) == 4
    want = None
    for layout in ("kohya", "peft", "diffusers", "diffusers018"):
        ck, truth = _checkpoint(sd, layout, wide)
        mods, rep = RL.parse_adapter(sd, ck, targets="transformer")
        assert sorted(mods) == sorted(truth) == sorted(R.attention_projections(sd) + wide) and rep["dropped"] == []
        for p, (d, u, a) in truth.items():
            assert mods[p][0].dim() == 2 and torch.equal(mods[p][0], d) and torch.equal(mods[p][1], u) and mods[p][2] == a
        want = want or sorted(mods)
        assert sorted(mods) == want
        with pytest.raises(ValueError) as e:                            # the default call still refuses, and says how to opt in
            RL.parse_adapter(sd, ck)
        assert all(p in str(e.value) for p in wide) and "lora_path=" in str(e.value) and 'targets="transformer"' in str(e.value)


def test_the_wider_set_still_refuses_by_name(sd):
    conv1 = next(k[:-7] for k in sd if k.endswith(".resnets.0.conv1.weight"))
    temb = next(k[:-7] for k in sd if k.endswith(".time_emb_proj.weight"))
    ck, _ = R.synthetic_adapter(sd, rank=4, seed=3, extra=F.wide_modules(sd) + [conv1, temb])
    with pytest.raises(ValueError) as e:
        RL.parse_adapter(sd, ck, targets="transformer")
    assert conv1 in str(e.value) and temb in str(e.value) and "lora_path=" in str(e.value) and ".ff.net.2'" not in str(e.value)
    mods, rep = RL.parse_adapter(sd, ck, attention_only=True, targets="transformer")
    assert sorted(rep["dropped"]) == sorted([conv1, temb]) and len(mods) == len(R.attention_projections(sd)) + len(F.wide_modules(sd))
    with pytest.raises(ValueError, match="targets must be one of"):
        RL.parse_adapter(sd, ck, targets="everything")
    # rank_layout's limits are what they were: the widest module of an adapter sets its block, four adapters, 128 rank columns
    big = {f"ad{l}": RL.parse_adapter(sd, R.synthetic_adapter(sd, rank=40, seed=l, extra=F.wide_modules(sd))[0], targets="transformer")[0] for l in range(3)}
    with pytest.raises(ValueError, match="144 rank columns.*128"):
        RL.rank_layout(big)
    assert RL.rank_layout({k: big[k] for k in ("ad0", "ad1")})[3] == 96


def test_merged_delta_and_concatenation_cover_the_four_modules(sd):
    ck, _ = R.synthetic_adapter(sd, rank=4, alpha=2.0, seed=3, extra=F.wide_modules(sd))
    adapters = {"A": RL.parse_adapter(sd, ck, targets="transformer")[0]}
    from rich_text_to_image_amd.lora import merge_lora
    merged, _ = merge_lora(sd, ck, 0.7)
    for path in F.wide_modules(sd):
        W = sd[path + ".weight"]
        down, up, aor, col = RL.concat_module(adapters, path, W[0].numel(), W.shape[0])
        got = (up.double() * (0.7 * aor.double())) @ down.double()
        assert torch.allclose(got, RL.merged_delta(adapters, path, [0.7]), rtol=0, atol=1e-12)
        assert torch.allclose(W.double().flatten(1) + got, merged[path + ".weight"].double().flatten(1), rtol=0, atol=2e-6)


@pytest.mark.parametrize("cfg", [TINY_SD_CONFIG, TINY_XL_CONFIG], ids=["sd", "xl"])
def test_weight_table_with_lora_targets(cfg):
    """lora_targets = 0 is the table of an engine built without the argument; 1 adds the three slots of the four modules, 2-D, in the
    main UNet only."""
    from rich_text_to_image_amd.engine import Engine, RtError
    today = Engine(cfg, 16, 16, device=-1, controlnet={}, lora_rank=32).weight_table()
    assert Engine(cfg, 16, 16, device=-1, controlnet={}, lora_rank=32, lora_targets=0).weight_table() == today
    wide = Engine(cfg, 16, 16, device=-1, controlnet={}, lora_rank=32, lora_targets=1).weight_table()
    assert [n for n in wide if n in today] == today
    sd = random_state_dict(cfg, seed=0)
    want = {}
    for p in F.wide_modules(sd):
        W = sd[p + ".weight"]
        want.update({f"lora.{p}.down.weight": (32, W[0].numel()), f"lora.{p}.up.weight": (W.shape[0], 32), f"lora.{p}.alpha_over_rank": (32,)})
    new = [n for n in wide if n not in today]
    assert dict(new) == want and len(new) == len(want) and not any("controlnet" in n for n, _ in new)
    for kw in (dict(lora_rank=32, lora_targets=2), dict(lora_rank=32, lora_targets=-1), dict(lora_rank=0, lora_targets=1)):
        with pytest.raises(RtError):
            Engine(cfg, 16, 16, device=-1, **kw)


def test_the_facade_asks_for_the_wide_engine_only_when_an_adapter_needs_it():
    from rich_text_to_image_amd.unet import HipUNet2DConditionModel
    sd = random_state_dict(TINY_XL_CONFIG, seed=11)
    u = HipUNet2DConditionModel(TINY_XL_CONFIG, sd)
    full, _ = R.synthetic_adapter(sd, rank=4, seed=3, extra=F.wide_modules(sd))
    attn, _ = R.synthetic_adapter(sd, rank=4, seed=3)
    u.load_regional_loras({"a": attn}, targets="transformer")
    assert (u.lora_rank, u.lora_targets) == (16, 0)
    u.load_regional_loras({"a": attn, "f": full}, targets="transformer")
    assert (u.lora_rank, u.lora_targets) == (32, 1)
    u.load_regional_loras({"f": full}, attention_only=True)
    assert (u.lora_rank, u.lora_targets) == (16, 0)
    with pytest.raises(ValueError, match="targets must be one of"):
        u.load_regional_loras({"f": full}, targets="all")
    u.unload_regional_loras()
    assert (u.lora_rank, u.lora_targets) == (0, 0)


def test_the_cli_flag():
    """--region_lora_targets: default attention, the two choices, anything else ends the parse."""
    from rich_text_to_image_amd import sample
    p = sample.build_parser()
    assert p.parse_args([]).region_lora_targets == "attention"
    for v in ("attention", "transformer"):
        assert p.parse_args(["--region_lora", "x.safetensors:0", "--region_lora_targets", v]).region_lora_targets == v
    with pytest.raises(SystemExit):
        p.parse_args(["--region_lora_targets", "everything"])


def test_an_engine_without_the_slots_refuses_a_wide_adapter():
    """The direct Engine API: adapters parsed with targets="transformer" on an engine built with lora_targets=0 would run half applied."""
    from rich_text_to_image_amd.engine import Engine
    sd = random_state_dict(TINY_XL_CONFIG, seed=11)
    ck, _ = R.synthetic_adapter(sd, rank=4, seed=3, extra=F.wide_modules(sd))
    e = Engine(TINY_XL_CONFIG, 16, 16, device=-1, lora_rank=16)
    try:
        with pytest.raises(ValueError, match="ff.net.0.proj"):
            e.bind_regional_loras({"A": RL.parse_adapter(sd, ck, targets="transformer")[0]})
    finally:
        e.close()


# ---------------------------------------------------------------------------------------------------------------- the bar
@pytest.fixture(scope="module")
def cases():
    out = []
    for case in F.GEGLU_CASES:
        inp = F.geglu_inputs(case)
        out.append((case, inp) + F.geglu_ref(inp))
    return out


def test_the_gates_span_both_sides_of_the_clamp(cases):
    for case, inp, ref, bar in cases:
        g = F.emulate_geglu(inp, pre=True)
        gates = torch.cat([v[1].flatten() for v in g.values()])
        assert float(gates.max()) > 4.25 and float(gates.min()) < -4.25 and float((gates.abs() < 4.25).float().mean()) > 0.5, case["name"]


def test_honest_emulation_is_within_the_bar(cases):
    for case, inp, ref, bar in cases:
        worst, share = R.worst_and_share(F.emulate_geglu(inp), ref, bar)
        zv, zg = F.split_packed(inp["Z"])
        far, _ = R.worst_and_share(F.bf(zv * F.gelu_poly(zg)), ref, bar)
        print(f"{case['name']}: honest emulation worst / bar {worst:.3f}; the base projection alone (no term) {far:.1f}")
        assert worst <= 1.0, (case["name"], share)
        assert far > 50.0
        for b, s in enumerate(inp["scales"]):
            if not any(s):
                assert float(bar[b].max()) == 0.0


def test_accumulation_allowance_is_the_measured_one():
    got = {case["name"]: F.measured_acc_units(case) for case in F.GEGLU_CASES}
    print("fp32 accumulation error of the emulation in units of 2^-24 S:", {k: round(v, 3) for k, v in got.items()})
    worst = max(got.values())
    assert worst <= F.GEGLU_ACC_UNITS <= 2 * worst and F.GPU_GEGLU_ACC_UNITS == 2 * F.GEGLU_ACC_UNITS


@pytest.mark.parametrize("mutant", F.MUTANTS)
def test_a_faulty_kernel_exceeds_the_bar(cases, mutant):
    factors = {case["name"]: R.worst_and_share(F.emulate_geglu(inp, mutant=mutant), ref, bar)[0] for case, inp, ref, bar in cases}
    print(f"{mutant}: worst / bar per case {dict((k, round(v, 2)) for k, v in factors.items())}")
    assert max(factors.values()) > 2.0, factors


def test_scale_after_rounding_is_reported(cases):
    """bf16(f bf16(T)) instead of bf16(f T): a second rounding of the same size as the first - it may stay within the bar; printed."""
    for case, inp, ref, bar in cases:
        print(f"scale applied after the rounding, {case['name']}: worst / bar {R.worst_and_share(F.emulate_geglu(inp, mutant='scale_after_rounding'), ref, bar)[0]:.3f}")


# ---------------------------------------------------------------------------------------------------------------- end to end
STREAM_SCALES = ((0.7, 0.0), (0.0, 1.0), (0.5, 0.8))      # what the adapted streams of the GPU forward test run at


@pytest.mark.parametrize("which", ["sd", "xl"])
def test_the_forward_cases_discriminate(which):
    """The merged oracle with the four modules left out of the merge is at least three forward bars from the full merged oracle, at every
    scale pair the GPU forward test uses: an engine that ignored them could not pass it."""
    sd, cks, attn = F.full_adapters(which)
    c = forward_case(which)
    added = {"text_embeds": c["pooled"][2:3], "time_ids": c["tid"]} if c["xl"] else None
    scales = list(STREAM_SCALES)
    full, part = R.lora_oracle(c["cfg"], sd, cks, scales), R.lora_oracle(c["cfg"], sd, attn, scales)
    with torch.no_grad():
        for s in scales:
            d = rel_l2(part.forward(c["lat"], c["t"], c["emb"][2:3], added)[0], full.forward(c["lat"], c["t"], c["emb"][2:3], added)[0])
            print(f"{which} scales {s}: the merge without ff / proj_in / proj_out is {d:.3e} from the full merge ({d / FORWARD_BAR:.1f} bars)")
            assert d >= 3 * FORWARD_BAR, s
