"""Regional LoRA without a GPU: the bar of tests/regional_lora_ref.py passes an honest kernel's emulation and catches seven faulty ones,
the accumulation allowance is the measured one, and the host logic of rich-text-to-image_amd/regional_lora.py - concatenation along the
rank, the four key layouts, the refusals, the slot-scale matrix, the packed layout - and the weight table of an engine with lora_rank."""
import math

import pytest
import torch

import regional_lora_ref as R
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict
from rich_text_to_image_amd import regional_lora as RL
from rich_text_to_image_amd.lora import merge_lora

MUTANTS = ("neighbour_scale", "no_alpha_over_rank", "pad_column_as_data", "headpad_rows_nonzero", "no_qscale", "untransposed")


@pytest.fixture(scope="module")
def cases():
    out = []
    for case in R.OP_CASES:
        inp = R.op_inputs(case)
        out.append((case, inp) + R.op_ref(inp, case["form"]))
    return out


def test_honest_emulation_is_within_the_bar(cases):
    for case, inp, ref, bar in cases:
        worst, share = R.worst_and_share(R.emulate(inp, case["form"]), ref, bar)
        far, _ = R.worst_and_share(inp["Y"], ref, bar)
        print(f"{case['name']}: honest emulation worst / bar {worst:.3f}; the input itself {far:.1f}")
        assert worst <= 1.0, (case["name"], share)
        assert far > 50.0
        for b, s in enumerate(inp["scales"]):
            if not any(s):
                assert float(bar[b].max()) == 0.0 and torch.equal(ref[b], inp["Y"][b].double())


def test_accumulation_allowance_is_the_measured_one():
    """ACC_UNITS covers the measured figure and is not more than twice it."""
    got = {case["name"]: R.measured_acc_units(case) for case in R.OP_CASES}
    print("fp32 accumulation error of the emulation in units of 2^-24 S:", {k: round(v, 3) for k, v in got.items()})
    worst = max(got.values())
    assert worst <= R.ACC_UNITS <= 2 * worst and R.GPU_ACC_UNITS == 2 * R.ACC_UNITS


@pytest.mark.parametrize("mutant", MUTANTS)
def test_a_faulty_kernel_exceeds_the_bar(cases, mutant):
    factors = {}
    for case, inp, ref, bar in cases:
        if mutant == "untransposed" and case["form"] != "bf16_t":
            continue
        factors[case["name"]] = R.worst_and_share(R.emulate(inp, case["form"], mutant=mutant), ref, bar)[0]
    print(f"{mutant}: worst / bar per case {dict((k, round(v, 2)) for k, v in factors.items())}")
    assert max(factors.values()) > 2.0, factors


def test_scale_after_rounding_is_reported(cases):
    """bf16(f bf16(T)) instead of bf16(f T): a second rounding of the same size as the first - it may stay within the bar; printed."""
    for case, inp, ref, bar in cases:
        print(f"scale applied after the rounding, {case['name']}: worst / bar {R.worst_and_share(R.emulate(inp, case['form'], mutant='scale_after_rounding'), ref, bar)[0]:.3f}")


# ---------------------------------------------------------------------------------------------------------------- host logic
@pytest.fixture(scope="module")
def sd():
    return random_state_dict(TINY_XL_CONFIG, seed=11)


def _parsed(sd, n, ranks=(4, 8, 3, 16)):
    out, cks = {}, []
    for l in range(n):
        ck, _ = R.synthetic_adapter(sd, rank=ranks[l], alpha=None if l % 2 else ranks[l] / 2.0, seed=10 + l, layout="peft" if l % 2 else "kohya")
        cks.append(ck)
        out[f"ad{l}"] = RL.parse_adapter(sd, ck)[0]
    return out, cks


@pytest.mark.parametrize("n", [1, 2, 3, 4])
def test_concatenation_along_the_rank_is_the_sum_of_the_adapters(sd, n):
    """sum_j f_j up[:, j] down[j, :] over the concatenated tables = sum_l s_l (alpha_l / r_l) B_l A_l in fp64, for every projection; and
    merging with lora.merge_lora at those scales gives W + that."""
    adapters, cks = _parsed(sd, n)
    scales = [0.7, -0.4, 1.3, 0.2][:n]
    layout = RL.rank_layout(adapters)
    assert layout[3] == sum(RL.pad_rank(r) for r in (4, 8, 3, 16)[:n]) and layout[3] % 16 == 0
    merged = sd
    for ck, s in zip(cks, scales):
        merged, _ = merge_lora(merged, ck, s)
    for path in R.attention_projections(sd):
        W = sd[path + ".weight"]
        down, up, aor, col = RL.concat_module(adapters, path, W.shape[1], W.shape[0], layout)
        f = torch.tensor(scales + [0.0] * (4 - n), dtype=torch.float64)[col.long()] * aor.double()
        got = (up.double() * f) @ down.double()
        want = RL.merged_delta(adapters, path, scales)
        assert torch.allclose(got, want, rtol=0, atol=1e-12)
        assert torch.allclose(W.double() + want, merged[path + ".weight"].double(), rtol=0, atol=2e-6)
        pads = aor == 0
        assert float(down[pads].abs().max() if pads.any() else 0) == 0.0 and float(up[:, pads].abs().max() if pads.any() else 0) == 0.0


def test_the_four_key_layouts_resolve_to_the_same_modules(sd):
    want = None
    for layout in ("kohya", "peft", "diffusers", "diffusers018"):
        ck, truth = R.synthetic_adapter(sd, rank=4, seed=3, layout=layout)
        mods, rep = RL.parse_adapter(sd, ck)
        assert sorted(mods) == sorted(truth) == sorted(R.attention_projections(sd)) and rep["dropped"] == []
        for p, (d, u, a) in truth.items():
            assert torch.equal(mods[p][0], d) and torch.equal(mods[p][1], u) and mods[p][2] == a
        want = want or sorted(mods)
        assert sorted(mods) == want
        assert (len(rep["alpha_default"]) == 0) == (layout == "kohya")


def test_refusals_name_what_they_refuse(sd):
    ff = "down_blocks.1.attentions.0.transformer_blocks.0.ff.net.2"
    pin = "down_blocks.1.attentions.0.proj_in"
    ck, _ = R.synthetic_adapter(sd, rank=4, seed=3, extra=(ff, pin))
    with pytest.raises(ValueError) as e:
        RL.parse_adapter(sd, ck)
    assert ff in str(e.value) and pin in str(e.value) and "lora_path=" in str(e.value)
    mods, rep = RL.parse_adapter(sd, ck, attention_only=True)
    assert sorted(rep["dropped"]) == sorted([ff, pin]) and ff not in mods and len(mods) == len(R.attention_projections(sd))
    ck["lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight"] = torch.zeros(4, 8)
    assert RL.parse_adapter(sd, ck, attention_only=True)[1]["text_encoder"] == ["lora_te_text_model_encoder_layers_0_mlp_fc1.lora_down.weight"]
    five, _ = _parsed(sd, 4)
    five["ad4"] = five["ad0"]
    with pytest.raises(ValueError, match="5 regional adapters.*4"):
        RL.rank_layout(five)
    big = {f"ad{l}": RL.parse_adapter(sd, R.synthetic_adapter(sd, rank=40, seed=l)[0])[0] for l in range(3)}
    with pytest.raises(ValueError, match="144 rank columns.*128"):
        RL.rank_layout(big)


def test_merge_lora_is_what_it_was(sd):
    """lora.merge_lora after the key parsing moved into resolve_targets: W + scale (alpha / rank) up @ down, the same report."""
    ck, truth = R.synthetic_adapter(sd, rank=4, alpha=2.0, seed=3)
    ck["lora_te_x.lora_down.weight"] = torch.zeros(4, 8)
    out, rep = merge_lora(sd, ck, 0.6)
    assert set(rep) == {"merged", "text_encoder", "alpha_default"} and rep["text_encoder"] == ["lora_te_x.lora_down.weight"] and rep["alpha_default"] == []
    assert rep["merged"] == [p + ".weight" for p in truth]
    for p, (d, u, a) in truth.items():
        assert torch.equal(out[p + ".weight"], (sd[p + ".weight"].float() + 0.6 * (a / 4) * (u @ d)).to(sd[p + ".weight"].dtype))
    assert all(torch.equal(out[k], v) for k, v in sd.items() if k[:-7] not in truth)


def test_slot_scale_matrix():
    """[negative, regions ..., base]: `scale` is every slot's default, regions= and negative= override it."""
    one = ["style"]
    assert RL.slot_scales(one, 0, scale=0.7) == [[0.7, 0, 0, 0], [0.7, 0, 0, 0]]                     # a plain request: [negative, base]
    assert RL.slot_scales(one, 0, scale=0.7, negative=0.0) == [[0, 0, 0, 0], [0.7, 0, 0, 0]]
    assert RL.slot_scales(one, 2, scale=0.0, regions={1: 1.0}) == [[0] * 4, [0] * 4, [1.0, 0, 0, 0], [0] * 4]
    two = ["a", "b"]
    got = RL.slot_scales(two, 2, scale={"a": 0.5}, regions={0: {"b": 1.0}}, negative={"a": 0.0})
    assert got == [[0, 0, 0, 0], [0, 1.0, 0, 0], [0.5, 0, 0, 0], [0.5, 0, 0, 0]]
    with pytest.raises(ValueError, match="region 2 is outside this request's 2 regions"):
        RL.slot_scales(one, 2, regions={2: 1.0})
    with pytest.raises(ValueError, match="2 adapters are loaded"):
        RL.slot_scales(two, 1, scale=0.5)
    with pytest.raises(ValueError, match="no regional adapter named"):
        RL.slot_scales(two, 1, scale={"c": 0.5})
    with pytest.raises(ValueError, match="finite"):
        RL.slot_scales(one, 0, scale=float("nan"))


def test_packed_layout():
    """`up` rows of to_q / to_k / to_v head-padded with zero rows, to_q's times d^-1/2 log2 e; `down` columns of to_out.0 head-padded."""
    H, d, DP, r, K = 3, 40, 64, 16, 24
    g = torch.Generator().manual_seed(0)
    down, up = torch.randn(r, K, generator=g), torch.randn(H * d, r, generator=g)
    for leaf, s in (("attn1.to_q", d ** -0.5 * math.log2(math.e)), ("attn2.to_k", 1.0), ("attn1.to_v", 1.0)):
        dp, upk = RL.pack_module(down, up, leaf, H, d, DP)
        assert torch.equal(dp, down.to(torch.bfloat16)) and upk.shape == (H * DP, r)
        u3 = upk.reshape(H, DP, r)
        assert torch.equal(u3[:, :d].reshape(H * d, r), (up * s).to(torch.bfloat16)) and float(u3[:, d:].abs().max()) == 0.0
    down_o, up_o = torch.randn(r, H * d, generator=g), torch.randn(K, r, generator=g)
    dp, upk = RL.pack_module(down_o, up_o, "attn2.to_out.0", H, d, DP)
    d3 = dp.reshape(r, H, DP)
    assert torch.equal(upk, up_o.to(torch.bfloat16)) and torch.equal(d3[:, :, :d].reshape(r, H * d), down_o.to(torch.bfloat16)) and float(d3[:, :, d:].abs().max()) == 0.0


# ---------------------------------------------------------------------------------------------------------------- the weight table
@pytest.mark.parametrize("cfg", [TINY_SD_CONFIG, TINY_XL_CONFIG], ids=["sd", "xl"])
def test_weight_table_with_lora_rank(cfg):
    """A weight-table-only engine with lora_rank = 32 lists exactly the base table plus the three lora.* slots of each of the eight
    attention projections per transformer block of the main UNet - none under controlnet. - with the factors' raw shapes."""
    from rich_text_to_image_amd.engine import Engine
    base = Engine(cfg, 16, 16, device=-1, controlnet={}).weight_table()
    with_lora = Engine(cfg, 16, 16, device=-1, controlnet={}, lora_rank=32).weight_table()
    assert [n for n in with_lora if not n[0].startswith("lora.")] == base
    sd = random_state_dict(cfg, seed=0)
    want = {}
    for p in R.attention_projections(sd):
        N, K = sd[p + ".weight"].shape
        want.update({f"lora.{p}.down.weight": (32, K), f"lora.{p}.up.weight": (N, 32), f"lora.{p}.alpha_over_rank": (32,)})
    got = dict(n for n in with_lora if n[0].startswith("lora."))
    assert got == want and not any("controlnet" in n for n in got)
    assert len(got) == len([n for n in with_lora if n[0].startswith("lora.")])
    assert Engine(cfg, 16, 16, device=-1, lora_rank=0).weight_table() == Engine(cfg, 16, 16, device=-1).weight_table()
    from rich_text_to_image_amd.engine import RtError
    for bad in (8, 24, 144, -16):
        with pytest.raises(RtError):
            Engine(cfg, 16, 16, device=-1, lora_rank=bad)
