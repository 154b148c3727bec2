"""ControlNet without a GPU: the checkpoint loader and its refusals, the command-line grammar, the hint's preprocessing, the weight table,
and the CPU references of tests/controlnet_ref.py against each other - the restatement with zero-valued zero convolutions IS the plain
oracle, and the inputs of the GPU tests discriminate: a dropped residual or an embedder fault cannot pass a bar."""
import functools

import numpy as np
import pytest
import torch

import controlnet_ref as R
from freeu_ref import FORWARD_BAR, oracle_streams
from oracle.shapes import weight_shapes
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet


# ---------------------------------------------------------------------------------------------------------------- loader
@pytest.mark.parametrize("cfg", [TINY_XL_CONFIG, TINY_SD_CONFIG], ids=["xl", "sd"])
def test_load_controlnet_reads_the_diffusers_layout(cfg, tmp_path):
    from rich_text_to_image_amd.controlnet import load_controlnet
    cn = R.control_state_dict(cfg, seed=3, embed_channels=(8, 16, 24, 40))
    got = load_controlnet(cn, cfg)
    assert got["embed_channels"] == (8, 16, 24, 40) and got["hint_channels"] == 3
    assert set(got["weights"]) == {"controlnet." + k for k in cn}
    assert all(torch.equal(got["weights"]["controlnet." + k], v) for k, v in cn.items())
    torch.save(cn, tmp_path / "cn.bin")
    again = load_controlnet(str(tmp_path / "cn.bin"), cfg)
    assert set(again["weights"]) == set(got["weights"])
    assert ("add_embedding.linear_1.weight" in cn) == (cfg["addition_embed_type"] == "text_time")


def test_load_controlnet_refuses_by_name():
    from rich_text_to_image_amd.controlnet import load_controlnet
    cfg = TINY_XL_CONFIG
    cn = R.control_state_dict(cfg, seed=3)
    with pytest.raises(ValueError, match=r"missing key controlnet_down_blocks\.4\.weight"):
        load_controlnet({k: v for k, v in cn.items() if k != "controlnet_down_blocks.4.weight"}, cfg)
    with pytest.raises(ValueError, match=r"left-over key controlnet_down_blocks\.9\.weight"):
        load_controlnet({**cn, "controlnet_down_blocks.9.weight": torch.zeros(128, 128, 1, 1)}, cfg)
    with pytest.raises(ValueError, match=r"down_blocks\.1\.resnets\.0\.conv1\.weight has shape .* does not belong to this UNet"):
        load_controlnet({**cn, "down_blocks.1.resnets.0.conv1.weight": torch.zeros(64, 48, 3, 3)}, cfg)
    with pytest.raises(ValueError, match="does not belong|missing key|left-over"):          # an SD ControlNet on the XL UNet
        load_controlnet(R.control_state_dict(TINY_SD_CONFIG, seed=3), cfg)
    with pytest.raises(ValueError, match=r"class_embedding\.linear_1\.weight: class-conditioned"):
        load_controlnet({**cn, "class_embedding.linear_1.weight": torch.zeros(4, 4)}, cfg)
    with pytest.raises(ValueError, match="guess_mode"):
        load_controlnet(cn, cfg, guess_mode=True)
    with pytest.raises(ValueError, match="global_pool_conditions"):
        load_controlnet(cn, cfg, global_pool_conditions=True)
    with pytest.raises(ValueError, match="multiples of 8"):
        load_controlnet(R.control_state_dict(cfg, seed=3, embed_channels=(16, 32, 36, 64)), cfg)
    with pytest.raises(ValueError, match="not found"):
        load_controlnet("/nonexistent/controlnet.safetensors", cfg)


def test_load_controlnet_reads_a_directory_and_its_config(tmp_path):
    import json
    from rich_text_to_image_amd.controlnet import load_controlnet
    cn = R.control_state_dict(TINY_SD_CONFIG, seed=3)
    torch.save(cn, tmp_path / "diffusion_pytorch_model.bin")
    (tmp_path / "config.json").write_text(json.dumps({"global_pool_conditions": False}))
    assert load_controlnet(str(tmp_path), TINY_SD_CONFIG)["embed_channels"] == R.TINY_EMBED
    (tmp_path / "config.json").write_text(json.dumps({"global_pool_conditions": True}))
    with pytest.raises(ValueError, match="global_pool_conditions"):
        load_controlnet(str(tmp_path), TINY_SD_CONFIG)


def test_make_controlnet_tool_writes_a_loadable_checkpoint(tmp_path):
    from rich_text_to_image_amd.controlnet import load_controlnet
    from tools.make_controlnet import make_controlnet
    out = tmp_path / "cn.bin"
    make_controlnet("tiny_xl", str(out), seed=4)
    got = load_controlnet(str(out), TINY_XL_CONFIG)
    zc = [v for k, v in got["weights"].items() if "controlnet_down_blocks" in k or "controlnet_mid_block" in k]
    assert zc and all(bool(v.abs().sum() > 0) for v in zc)               # non-zero zero convolutions


# ---------------------------------------------------------------------------------------------------------------- grammar
def test_control_scale_parsing():
    from rich_text_to_image_amd.controlnet import control_from_request, parse_scale_args
    assert parse_scale_args(None) == dict(scale=1.0, regions={}, negative=None)
    assert parse_scale_args(["0.8"]) == dict(scale=0.8, regions={}, negative=None)
    assert parse_scale_args(["0.8", "negative:0", "1:0.25", "0:1.5"]) == dict(scale=0.8, regions={1: 0.25, 0: 1.5}, negative=0.0)
    assert parse_scale_args(["base:0.5", "2:-1"]) == dict(scale=0.5, regions={2: -1.0}, negative=None)
    assert parse_scale_args(0.7)["scale"] == 0.7
    for bad in (["x"], ["foo:1"], ["1:"], ["nan"], ["1:inf"], ["0.5", "base:0.6"], ["1:0.5", "1:0.6"], ["negative:1", "negative:2"], ["-1:0.5"]):
        with pytest.raises(ValueError):
            parse_scale_args(bad)
    kw = control_from_request({"image": "edges.png", "scale": ["0.9", "0:0"], "start": 0.1, "end": 0.7})
    assert kw == dict(image="edges.png", scale=0.9, regions={0: 0.0}, negative=None, start=0.1, end=0.7)
    for bad in ({"scale": 1.0}, {"image": "a.png", "strength": 1}, "a.png", {"image": "a.png", "start": "x"}):
        with pytest.raises(ValueError):
            control_from_request(bad)


def test_control_window_follows_the_guidance_fractions():
    from rich_text_to_image_amd.controlnet import control_window
    assert control_window(10, 0.0, 1.0) == list(range(10))
    assert control_window(10, 0.2, 0.6) == [2, 3, 4, 5]
    assert control_window(5, 0.2, 0.6) == [1, 2]
    assert control_window(3, 0.5, 1.0) == [2]
    assert control_window(4, 0.0, 0.1) == []


def test_set_control_checks_its_arguments():
    from rich_text_to_image_amd.controlnet import ControlNetMixin

    class Pipe(ControlNetMixin):
        pass
    p = Pipe()
    with pytest.raises(ValueError, match="no ControlNet loaded"):
        p.set_control(image=np.zeros((8, 8, 3), np.uint8))
    p.controlnet = dict(hint_channels=3, embed_channels=R.TINY_EMBED, weights={})
    img = np.zeros((8, 8, 3), np.uint8)
    for kw in (dict(image=None), dict(image=img, scale=float("nan")), dict(image=img, regions=[1.0]), dict(image=img, regions={-1: 1.0}),
               dict(image=img, regions={0: "x"}), dict(image=img, start=0.6, end=0.6), dict(image=img, start=-0.1), dict(image=img, end=1.5)):
        with pytest.raises(ValueError):
            p.set_control(**kw)
    assert p.control is None
    p.set_control(image=img, scale=0.8, regions={1: 0.25}, negative=0.0)
    assert p.control_scales(2, rich=False) == [0.0, 0.8]                                     # the plain pass: [negative, base]
    assert p.control_scales(4, rich=True) == [0.0, 0.8, 0.25, 0.8]                           # [negative, region 0, region 1, base]
    with pytest.raises(ValueError, match="region 1"):
        p.control_scales(3, rich=True)
    p.set_control(image=img)                                                                 # diffusers: the unconditional half is controlled too
    assert p.control_scales(2, rich=False) == [1.0, 1.0]
    p.clear_control()
    assert p.control_scales(2, rich=False) is None


# ---------------------------------------------------------------------------------------------------------------- hint
def test_preprocess_hint_geometry(tmp_path):
    from PIL import Image
    from rich_text_to_image_amd.controlnet import preprocess_hint
    a = np.zeros((40, 56, 3), np.uint8)
    a[:, 28:] = 255
    a[..., 2] = 51
    same = preprocess_hint(a, 40, 56)
    assert same.dtype == np.float32 and same.shape == (3, 40, 56) and same.flags["C_CONTIGUOUS"]
    assert np.array_equal(same, a.transpose(2, 0, 1).astype(np.float32) / 255)              # no resize: only converted
    big = preprocess_hint(a, 80, 112)
    assert big.shape == (3, 80, 112) and big.min() >= 0.0 and big.max() <= 1.0
    assert abs(float(big[0, :, :40].mean())) < 1e-3 and abs(float(big[0, :, 72:].mean()) - 1.0) < 1e-3 and np.allclose(big[2], 0.2)
    Image.fromarray(a).save(tmp_path / "h.png")
    assert np.array_equal(preprocess_hint(str(tmp_path / "h.png"), 40, 56), same)
    assert np.array_equal(preprocess_hint(Image.fromarray(a[..., 0]), 40, 56)[1], same[0])  # grey -> RGB
    for bad, h, w in ((a, 40, 60), (a.astype(np.float32), 40, 56), (a[..., :2], 40, 56), (str(tmp_path / "none.png"), 40, 56), (a, 0, 56)):
        with pytest.raises(ValueError):
            preprocess_hint(bad, h, w)


# ---------------------------------------------------------------------------------------------------------------- weight table
@pytest.mark.parametrize("cfg", [TINY_XL_CONFIG, TINY_SD_CONFIG], ids=["xl", "sd"])
def test_weight_table_is_the_reference_names_plus_the_controlnet(cfg):
    """A weight-table-only engine (no device): controlnet=None leaves the table as it is - exactly the reference's state_dict names, in
    the same order as ever - and a ControlNet appends exactly the names of its checkpoint under "controlnet.", shapes included."""
    from rich_text_to_image_amd.engine import Engine, RtError
    plain = Engine(cfg, 16, 16, device=-1)
    off = Engine(cfg, 16, 16, device=-1, controlnet=None)
    on = Engine(cfg, 16, 16, device=-1, controlnet=dict(embed_channels=R.TINY_EMBED))
    try:
        t0, t1, t2 = plain.weight_table(), off.weight_table(), on.weight_table()
        assert t1 == t0 and {n: tuple(s) for n, s in t0} == {n: tuple(s) for n, s in weight_shapes(cfg).items()}
        assert t2[:len(t0)] == t0
        cn = R.control_state_dict(cfg)
        assert {n: tuple(s) for n, s in t2[len(t0):]} == {"controlnet." + k: tuple(v.shape) for k, v in cn.items()}
        assert plain.trace_modules() == off.trace_modules() and not any(n.startswith("controlnet.") for n, _, _ in plain.trace_modules())
        names = [n for n, _, _ in on.trace_modules()]
        assert [n for n in names if not n.startswith("controlnet.")] == [n for n, _, _ in plain.trace_modules()]
        first = names.index("controlnet.hint_embedding")
        assert names[first - 1] == "mid_block.resnets.1" and names[first + 1] == "controlnet.conv_in" and "controlnet.mid" in names
        assert sum(n.startswith("controlnet.skip.") for n in names) == len(R.skip_channels(cfg))
        default = Engine(cfg, 16, 16, device=-1, controlnet={})
        try:
            assert dict(default.weight_table())["controlnet.controlnet_cond_embedding.blocks.5.weight"] == (256, 96, 3, 3)
        finally:
            default.close()
        with pytest.raises(ValueError):
            Engine(cfg, 16, 16, device=-1, controlnet=dict(embed_channels=(16, 32, 36, 64)))
    finally:
        plain.close(); off.close(); on.close()


# ---------------------------------------------------------------------------------------------------------------- the references
@functools.lru_cache(maxsize=None)
def _case(which):
    c = R.control_case(which)
    plain = oracle_streams(OracleUNet(c["cfg"], c["sd"]), c)
    outs, tr = R.traced_streams(R.ControlOracleUNet(c["cfg"], c["sd"], c["cn"], c["hint"], R.FORWARD_STREAM_SCALES), c)
    return c, plain, outs, tr


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_ref_with_zero_valued_zero_convolutions_is_the_plain_oracle(which):
    c, plain, _, _ = _case(which)
    o = R.ControlOracleUNet(c["cfg"], c["sd"], R.zeroed(c["cn"]), c["hint"], [1.0, 1.0, 1.0, 0.5])
    for k, (got, want) in enumerate(zip(oracle_streams(o, c), plain)):
        assert torch.equal(got, want), k


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_forward_cases_discriminate(which):
    """On the CPU references alone: every controlled stream's output is >= 10 x FORWARD_BAR from the uncontrolled oracle, the uncontrolled
    stream IS the plain oracle, and every controlnet.skip.{k} / controlnet.mid is >= 5 x the bar from the un-added tensor."""
    c, plain, outs, tr = _case(which)
    assert torch.equal(outs[0], plain[0])
    _, tr_plain = R.traced_streams(OracleUNet(c["cfg"], c["sd"]), c)
    for k in (1, 2, 3):
        d = R.rel_l2(outs[k], plain[k])
        print(f"{which} stream {k}: controlled vs plain oracle {d:.3f}")
        assert d >= 10 * FORWARD_BAR, (k, d)
    # the un-added tensors: the skips are the outputs of the modules that push them (the down path runs on un-added tensors)
    src = R.skip_sources(c["cfg"])
    for k in (1, 2):                      # (stream 3's un-added tensors depend on the injection: streams 1 and 2 carry the check)
        for j, name in enumerate(src):
            d = R.rel_l2(tr[k][f"controlnet.skip.{j}"], tr[k][name])
            assert d >= 5 * FORWARD_BAR, (k, j, d)
        d = R.rel_l2(tr[k]["controlnet.mid"], tr[k]["mid_block.resnets.1"])
        assert d >= 5 * FORWARD_BAR, (k, "mid", d)
        assert torch.equal(tr[k]["conv_in"], tr_plain[k]["conv_in"])


@pytest.mark.parametrize("h,w", [(16, 24), (32, 64)])
def test_embedder_bar_and_faults(h, w):
    """The bar (margin x emulation error) is a few bf16 roundings wide, and every injected embedder fault lies >= 5 x the bar away: a
    missing SiLU, a stride or a pad off by one, a dropped bias."""
    cn = R.control_state_dict(TINY_XL_CONFIG, seed=21)
    hint = R.make_hint(h, w)
    exact = R.embed_ref(cn, hint)
    assert tuple(exact.shape) == (32, h, w)
    bar = R.embed_bar(cn, hint, exact)
    print(f"embedder {8 * h} x {8 * w}: bar {bar:.3e} (rel-L2)")
    assert 2.0 ** -9 < bar < 16 * 2.0 ** -8
    faults = dict(no_silu_first=dict(no_silu_after="conv_in"), no_silu_last=dict(no_silu_after="blocks.5"), no_silu_mid=dict(no_silu_after="blocks.2"),
                  drop_bias_in=dict(drop_bias="conv_in"), drop_bias_out=dict(drop_bias="conv_out"), drop_bias_mid=dict(drop_bias="blocks.3"))
    for name, kw in faults.items():
        d = R.rel_l2(R.embed_ref(cn, hint, **kw), exact)
        assert d >= 5 * bar, (name, d, bar)
    # geometry faults change the grid: compare on the common top-left window (a kernel with such a fault writes SOMETHING at every pixel)
    for name, kw in dict(stride_1=dict(stride_all=1), pad_0=dict(pad=0), pad_2=dict(pad=2)).items():
        f = R.embed_ref(cn, hint, **kw)
        hh, ww = min(h, f.shape[1]), min(w, f.shape[2])
        d = R.rel_l2(f[:, :hh, :ww], exact[:, :hh, :ww])
        assert d >= 5 * bar, (name, d, bar)


def test_embedding_on_the_wrong_side_of_conv_in_is_visible():
    """The embedding added to the main UNet's conv_in output instead of the control copy's: the control copy's conv_in tensor is then
    >= 5 x the embedder bar from the right one (and the stream's output beyond the forward bar)."""
    c, _, outs, tr = _case("xl")
    bad_o, bad_tr = R.traced_streams(R.ControlOracleUNet(c["cfg"], c["sd"], c["cn"], c["hint"], R.FORWARD_STREAM_SCALES, fault="embedding_on_unet_conv_in"), c)
    bar = R.embed_bar(c["cn"], c["hint"])
    d = R.rel_l2(bad_tr[1]["controlnet.conv_in"], tr[1]["controlnet.conv_in"])
    assert d >= 5 * bar, (d, bar)
    assert R.rel_l2(bad_o[1], outs[1]) > FORWARD_BAR


def test_add_ref_bar_is_two_roundings():
    skip, r = R.add_inputs(3, 24, 32, 2)
    ref, bar = R.add_ref(skip, r, [0, 2], [0.6, -0.5])
    assert torch.equal(ref[1], skip[1].double()) and float(bar[1].max()) == 0.0
    assert bool((bar[0] <= 2.0 ** -10 * ref[0].abs() + 2.0 ** -24).all()) and bool((bar[0] >= 2.0 ** -11 * ref[0].abs()).all())
    honest = torch.addcmul(skip[[0, 2]].float(), r, torch.tensor([0.6, -0.5])[:, None, None]).half()      # fp32 arithmetic, one fp16 rounding
    assert bool(((honest.double() - ref[[0, 2]]).abs() <= bar[[0, 2]]).all())
    # the input itself (a dropped add) and a wrong sign are far outside
    assert float(((skip[[0, 2]].double() - ref[[0, 2]]).abs() > bar[[0, 2]]).double().mean()) > 0.9
