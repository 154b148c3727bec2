"""CPU side of the CLIP vision encoder (rich_text_to_image_amd/clip_vision_encoder.py, csrc/vision.hip): the attention bar of
tests/clip_vision_ref.py passes an honest kernel's arithmetic and catches three faulty ones; `preprocess` equals transformers'
CLIPImageProcessor geometry; the loader, the facade and the command line refuse what they must - and what they refused before."""
import json
import os

import numpy as np
import pytest
import torch

import clip_vision_ref as V
import ip_adapter_ref as R
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict

TINY = V.vision_config(V.ENCODER_CASES[0])


# ---------------------------------------------------------------------------------------------------------------- the attention bar
@pytest.fixture(scope="module")
def attn_cases():
    out = {}
    for case in V.ATTN_CASES:
        qkv = V.attn_inputs(*case)
        out[case] = (qkv, *V.attn_ref(qkv, *case))
    return out


@pytest.mark.parametrize("case", V.ATTN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bar_passes_an_honest_kernel(attn_cases, case):
    qkv, ref, bar = attn_cases[case]
    w = V.worst(V.emulate(qkv, *case), ref, bar)
    print(f"bidir attention bar, honest emulation {case}: worst ratio {w:.3f}")
    assert w < 1.0


@pytest.mark.parametrize("case", V.ATTN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bar_catches_faulty_kernels(attn_cases, case):
    qkv, ref, bar = attn_cases[case]
    B, H, N, d = case
    w_pad = V.worst(V.emulate(qkv, *case, pad_key=True), ref, bar)
    w_drop = V.worst(V.emulate(qkv, *case, drop_last=True), ref, bar)
    w_scale = V.worst(V.emulate(qkv, *case, padded_scale=True), ref, bar)
    print(f"bidir attention bar, faulty emulations {case}: padding key scored {w_pad:.1f}, last key dropped {w_drop:.1f}, padded scale {w_scale:.1f}")
    assert w_pad > 1.0 and w_drop > 1.0
    if V.padded(d) != d:                       # d = 64 is its own padded width: that mutation is the honest kernel there
        assert w_scale > 1.0
    else:
        assert w_scale < 1.0


# ---------------------------------------------------------------------------------------------------------------- preprocess
@pytest.mark.parametrize("hw", [(300, 200), (200, 300), (224, 224), (37, 91)])
def test_preprocess_matches_transformers(hw):
    from transformers import CLIPImageProcessorPil
    from PIL import Image
    from rich_text_to_image_amd.clip_vision_encoder import CLIP_MEAN, CLIP_STD, preprocess
    arr = V.synthetic_image(*hw)
    size = 224
    proc = CLIPImageProcessorPil(size={"shortest_edge": size}, crop_size={"height": size, "width": size})
    # the geometry alone: uint8 out of transformers' resize + centre crop
    crop_ref = proc(Image.fromarray(arr), do_rescale=False, do_normalize=False, return_tensors="pt")["pixel_values"][0]
    got = preprocess(arr, size)
    assert got.dtype == np.uint8 and got.shape == (size, size, 3)
    assert torch.equal(torch.from_numpy(got.copy()).permute(2, 0, 1).to(crop_ref.dtype), crop_ref)
    # a PIL image and a file give the same crop
    assert np.array_equal(preprocess(Image.fromarray(arr), size), got)
    # the patchify formula on the crop = pixel_values
    pv = proc(Image.fromarray(arr), return_tensors="pt")["pixel_values"][0]
    mine = (torch.from_numpy(got.copy()).double() / 255.0 - torch.tensor(CLIP_MEAN, dtype=torch.float64)) / torch.tensor(CLIP_STD, dtype=torch.float64)
    err = (mine.permute(2, 0, 1) - pv.double()).abs().max().item()
    print(f"preprocess {hw}: crop equal, max |patchify formula - pixel_values| = {err:.2e}")
    assert err < 1e-6
    assert tuple(proc.image_mean) == pytest.approx(CLIP_MEAN) and tuple(proc.image_std) == pytest.approx(CLIP_STD)


def test_preprocess_reads_files_and_refuses_other_things(tmp_path):
    from PIL import Image
    from rich_text_to_image_amd.clip_vision_encoder import preprocess
    arr = V.synthetic_image(60, 90)
    Image.fromarray(arr).save(tmp_path / "a.png")
    assert np.array_equal(preprocess(str(tmp_path / "a.png"), 56), preprocess(arr, 56))
    (tmp_path / "b.png").write_text("not a picture")
    for bad in (str(tmp_path / "none.png"), str(tmp_path / "b.png"), arr.astype(np.float32), arr[..., :2], np.zeros((0, 4, 3), np.uint8)):
        with pytest.raises(ValueError):
            preprocess(bad, 56)


# ---------------------------------------------------------------------------------------------------------------- loader
def _write_encoder(path, cfg=TINY, drop=None, fmt="safetensors", preprocessor=None):
    from rich_text_to_image_amd.clip_vision_encoder import empty_state_dict
    os.makedirs(path, exist_ok=True)
    if cfg is not None:
        with open(os.path.join(path, "config.json"), "w") as f:
            json.dump(cfg, f)
    sd = {k: v for k, v in empty_state_dict(TINY).items() if k != drop}
    if fmt == "safetensors":
        from safetensors.torch import save_file
        save_file(sd, os.path.join(path, "model.safetensors"))
    elif fmt == "bin":
        torch.save(sd, os.path.join(path, "pytorch_model.bin"))
    if preprocessor is not None:
        with open(os.path.join(path, "preprocessor_config.json"), "w") as f:
            json.dump(preprocessor, f)
    return str(path)


def test_state_dict_keys_are_transformers_keys():
    from rich_text_to_image_amd.clip_vision_encoder import empty_state_dict
    ref = V.random_vision_model(V.ENCODER_CASES[0]).state_dict()
    mine = empty_state_dict(TINY)
    assert {k: tuple(v.shape) for k, v in mine.items()} == {k: tuple(v.shape) for k, v in ref.items() if not k.endswith("position_ids")}


def test_loader_reads_a_directory_and_refuses_bad_ones(tmp_path):
    from rich_text_to_image_amd.clip_vision_encoder import CLIP_MEAN, LazyImageEncoder, read_image_encoder
    sd, cfg, mean, std, size = read_image_encoder(_write_encoder(tmp_path / "ok"))
    assert cfg["hidden_size"] == 160 and mean == CLIP_MEAN and size == 56 and "visual_projection.weight" in sd
    sd, cfg, mean, std, size = read_image_encoder(_write_encoder(tmp_path / "bin", fmt="bin", preprocessor=dict(
        image_mean=[0.5, 0.5, 0.5], image_std=[0.25, 0.25, 0.25], crop_size={"height": 56, "width": 56})))
    assert mean == (0.5, 0.5, 0.5) and std == (0.25, 0.25, 0.25)
    lazy = LazyImageEncoder(tmp_path / "ok")                         # host-side object: nothing on a GPU yet
    assert lazy.projection_dim == 48 and lazy.S == 56
    text_cfg = dict(model_type="clip_text_model", hidden_size=160, num_attention_heads=2, num_hidden_layers=3, intermediate_size=320, vocab_size=1000)
    for path, word in ((str(tmp_path / "nowhere"), "nowhere"),
                       (_write_encoder(tmp_path / "nocfg", cfg=None), "config.json"),
                       (_write_encoder(tmp_path / "text", cfg=text_cfg), "not a CLIP vision config"),
                       (_write_encoder(tmp_path / "noweights", fmt=None), "model.safetensors"),
                       (_write_encoder(tmp_path / "missing", drop="vision_model.encoder.layers.1.mlp.fc2.bias"), "vision_model.encoder.layers.1.mlp.fc2.bias"),
                       (_write_encoder(tmp_path / "big", cfg=dict(TINY, image_size=364)), "tokens"),                 # 26^2 + 1 = 677 > 640
                       (_write_encoder(tmp_path / "wide", cfg=dict(TINY, hidden_size=288)), "head dim"),             # 144 per head
                       (_write_encoder(tmp_path / "crop", preprocessor=dict(crop_size=64)), "crop_size")):
        with pytest.raises(ValueError) as e:
            read_image_encoder(path)
        assert word in str(e.value), (path, str(e.value))


# ---------------------------------------------------------------------------------------------------------------- facade / command line
def _pipeline(which="sd"):
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    cfg = TINY_XL_CONFIG if which == "xl" else TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=3)
    m = RegionDiffusionXL(device=0, unet_state_dict=sd, config=cfg) if which == "xl" else RegionDiffusion(0, unet_state_dict=sd, config=cfg)
    return m, cfg, sd


@pytest.mark.parametrize("which", ["xl", "sd"])
def test_facade_validation_of_pictures(which, tmp_path):
    m, cfg, sd = _pipeline(which)
    arr = V.synthetic_image(70, 60)
    enc_dir = _write_encoder(tmp_path / "enc")
    with pytest.raises(ValueError):                                   # no adapter
        m.set_image_prompts(base=dict(image=arr))
    m.load_ip_adapter(R.synthetic_checkpoint(cfg, sd, T=4, E=48)[0])
    assert m.image_encoder is None
    with pytest.raises(ValueError) as e:                              # no encoder
        m.set_image_prompts(base=dict(image=arr))
    assert "image encoder" in str(e.value) and m.image_prompts is None
    for bad in (str(tmp_path / "nowhere"), 3):
        with pytest.raises(ValueError):
            m.load_image_encoder(bad)
    assert m.image_encoder is None
    m.load_image_encoder(enc_dir)
    m.set_image_prompts(base=dict(image=arr, scale=0.5), regions={0: dict(embeds=torch.ones(48))})
    e = m.image_prompts["base"]
    assert e["scale"] == 0.5 and e["image"].dtype == torch.uint8 and tuple(e["image"].shape) == (56, 56, 3) and "_embeds" not in e
    for bad in (dict(base=dict(image=arr, embeds=torch.ones(48))), dict(base=dict(image=arr, tokens=torch.ones(2, cfg["cross_attention_dim"]))),
                dict(base=dict(image=arr, weight=1.0)), dict(base=dict(image=str(tmp_path / "none.png"))), dict(base=dict(image=arr.astype(np.float32))),
                dict(base=dict(image=arr, scale=float("inf"))), dict(base="image.png"), dict(regions={0: arr})):
        m.clear_image_prompts()
        with pytest.raises(ValueError):
            m.set_image_prompts(**bad)
        assert m.image_prompts is None
    m.unload_image_encoder()
    assert m.image_encoder is None
    with pytest.raises(ValueError):
        m.set_image_prompts(base=dict(image=arr))
    # an encoder whose projection_dim is not the adapter's E
    m.load_ip_adapter(R.synthetic_checkpoint(cfg, sd, T=4, E=24)[0])
    m.load_image_encoder(enc_dir)
    with pytest.raises(ValueError) as e:
        m.set_image_prompts(base=dict(image=arr))
    assert "projection_dim" in str(e.value) and "48" in str(e.value) and "24" in str(e.value)
    m.set_image_prompts(base=dict(embeds=torch.ones(24)))             # embeddings do not need the encoder to fit


def test_command_line_validation_of_pictures(tmp_path):
    from PIL import Image
    from rich_text_to_image_amd import sample
    from rich_text_to_image_amd.ip_adapter import image_prompts_from_specs, parse_embeds_arg, parse_image_arg
    assert parse_image_arg("a.png") == ("a.png", "base", 1.0)
    assert parse_image_arg("dir/a.JPG:2:0.35") == ("dir/a.JPG", 2, 0.35)
    assert parse_image_arg("a.jpeg:negative") == ("a.jpeg", "negative", 1.0)
    for bad in ("a.png:left", "a.png:1:much", "a.png:1:nan", "a.png:1:2:3", ":base", "a.pt", "a.png:-1", "a"):
        with pytest.raises(ValueError):
            parse_image_arg(bad)
    for bad in ("a.png", "a.pt:left", "a.pt:-1"):                     # the embedding parser refuses what it refused
        with pytest.raises(ValueError):
            parse_embeds_arg(bad)
    ip = image_prompts_from_specs(["a.pt:negative"], images=["cat.png:0", "sky.jpg:base:0.6"])
    assert ip["negative"] == dict(file="a.pt", scale=1.0) and ip["regions"] == {0: dict(image_file="cat.png", scale=1.0)}
    assert ip["base"] == dict(image_file="sky.jpg", scale=0.6)
    assert image_prompts_from_specs({"embeds": ["a.pt"], "images": [{"file": "c.png", "target": 1}]})["regions"] == {1: dict(image_file="c.png", scale=1.0)}
    for specs, images in ((["a.pt"], ["b.png"]), (None, ["a.png:1", "b.png:1"]), ({"embeds": ["a.pt:0"], "images": ["b.png:0"]}, None),
                          ({"pictures": ["b.png"]}, None), (None, [{"target": 1}])):
        with pytest.raises(ValueError):
            image_prompts_from_specs(specs, images=images)
    # main(): bad values end the run before any rank starts
    emb, ad, pic = tmp_path / "e.pt", tmp_path / "ip.bin", tmp_path / "x.png"
    torch.save(torch.zeros(24), emb)
    torch.save({}, ad)
    Image.fromarray(V.synthetic_image(40, 50)).save(pic)
    enc = _write_encoder(tmp_path / "enc")
    js = json.dumps({"ops": [{"insert": "a cat\n"}]})
    base = ["--rich_text_json", js, "--gpus", "2", "--dry_launch"]
    for argv, word in ((["--ip_images", str(pic), "--image_encoder", enc], "needs --ip_adapter"),
                       (["--ip_adapter", str(ad), "--ip_images", str(pic)], "needs --image_encoder"),
                       (["--ip_adapter", str(ad), "--image_encoder", str(tmp_path / "nowhere"), "--ip_images", str(pic)], "file not found"),
                       (["--ip_adapter", str(ad), "--image_encoder", enc, "--ip_images", str(tmp_path / "none.png")], "file not found"),
                       (["--ip_adapter", str(ad), "--image_encoder", enc, "--ip_images", f"{pic}:sky"], "TARGET"),
                       (["--ip_adapter", str(ad), "--image_encoder", enc, "--ip_images", f"{pic}:0:inf"], "SCALE"),
                       (["--ip_adapter", str(ad), "--image_encoder", enc, "--ip_images", str(emb)], "the file must be"),
                       (["--ip_adapter", str(ad), "--image_encoder", enc, "--ip_images", f"{pic}:0", "--ip_image_embeds", f"{emb}:0"], "two image prompts"),
                       (["--ip_adapter", str(ad), "--ip_image_embeds", str(pic)], "the file must be")):
        with pytest.raises(SystemExit) as e:
            sample.main(base + argv)
        assert word in str(e.value), (argv, str(e.value))
    req = tmp_path / "r.jsonl"
    req.write_text(json.dumps({"rich_text_json": {"ops": [{"insert": "a cat\n"}]}, "image_prompts": {"images": [f"{pic}:oops"]}}) + "\n")
    with pytest.raises(SystemExit) as e:
        sample.main(["--requests", str(req), "--ip_adapter", str(ad), "--image_encoder", enc, "--gpus", "2", "--dry_launch"])
    assert "line 1" in str(e.value) and "TARGET" in str(e.value)
    req.write_text(json.dumps({"rich_text_json": {"ops": [{"insert": "a cat\n"}]}, "image_prompts": {"images": [f"{pic}:1"]}}) + "\n")
    with pytest.raises(SystemExit) as e:                              # a request's picture without an encoder
        sample.main(["--requests", str(req), "--ip_adapter", str(ad), "--gpus", "2", "--dry_launch"])
    assert "needs --image_encoder" in str(e.value)
    # good lines: a request's own pictures and embeddings, the next one the flags'
    req.write_text(json.dumps({"rich_text_json": {"ops": [{"insert": "a cat\n"}]}, "image_prompts": {"images": [f"{pic}:1:0.5"], "embeds": [str(emb)]}}) + "\n" +
                   json.dumps({"rich_text_json": {"ops": [{"insert": "a dog\n"}]}}) + "\n")
    a = sample.build_parser().parse_args(["--requests", str(req), "--ip_adapter", str(ad), "--image_encoder", enc, "--ip_images", f"{pic}:base:0.25",
                                          "--ip_image_embeds", f"{emb}:negative"])
    a.freeu = None
    a.image_prompts = sample.check_ip_args(a)
    reqs = sample.build_requests(a)
    assert reqs[0]["image_prompts"]["regions"] == {1: dict(image_file=str(pic), scale=0.5)} and reqs[0]["image_prompts"]["base"] == dict(file=str(emb), scale=1.0)
    assert reqs[1]["image_prompts"]["base"] == dict(image_file=str(pic), scale=0.25) and reqs[1]["image_prompts"]["negative"] == dict(file=str(emb), scale=1.0)


def test_apply_specs_hands_pictures_to_the_pipeline(tmp_path):
    from PIL import Image
    from rich_text_to_image_amd.ip_adapter import apply_specs, image_prompts_from_specs
    m, cfg, sd = _pipeline("sd")
    m.load_ip_adapter(R.synthetic_checkpoint(cfg, sd, T=4, E=48)[0])
    pic = tmp_path / "x.png"
    Image.fromarray(V.synthetic_image(40, 50)).save(pic)
    parsed = image_prompts_from_specs(None, images=[f"{pic}:base:0.6"])
    with pytest.raises(ValueError):                                   # no encoder on the pipeline
        apply_specs(m, parsed)
    m.load_image_encoder(_write_encoder(tmp_path / "enc"))
    apply_specs(m, parsed)
    assert m.image_prompts["base"]["scale"] == 0.6 and tuple(m.image_prompts["base"]["image"].shape) == (56, 56, 3)


def test_library_refuses_without_gpu_state(lib):
    """The new operators are exported and refuse bad shapes on the host, before any launch (no GPU needed for a refusal)."""
    import ctypes as C
    for name in ("rt_op_patchify", "rt_op_vit_embed", "rt_op_bidir_attention"):
        assert hasattr(lib, name)
    buf = (C.c_char * 64)()
    p = C.cast(buf, C.c_void_p)
    for N, d in ((641, 80), (257, 136), (257, 84), (0, 80)):
        assert lib.rt_op_bidir_attention(p, p, p, 3 * 2 * d, p, 2 * d, 1, 2, N, d, C.c_float(0.1), None) != 0
    assert b"bidir attention" in lib.rt_op_last_error()
    assert lib.rt_op_layernorm(p, p, p, p, 4, 2056, C.c_float(1e-5), None) != 0
    assert b"2048" in lib.rt_op_last_error()
