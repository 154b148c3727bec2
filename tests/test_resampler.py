"""CPU side of the Resampler of the IP-Adapter "plus" checkpoints (rich_text_to_image_amd/resampler.py, csrc/resampler.hip): the attention
bar of tests/resampler_ref.py passes an honest split-key kernel's arithmetic and catches five faulty ones by a factor of ten; the loader
reads the plus layout, infers every dimension and names the key of anything unusable, and a linear checkpoint loads as before; entries
and the command-line tool; the bf16 chain against the fp64 Resampler."""
import os
import subprocess
import sys

import pytest
import torch

import ip_adapter_ref as R
import resampler_ref as RS
from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MUTATIONS = ("pad_key", "drop_last", "no_factors", "padded_scale", "no_latent_keys")


# ---------------------------------------------------------------------------------------------------------------- the attention bar
@pytest.fixture(scope="module")
def attn_cases():
    out = {}
    for case in RS.ATTN_CASES:
        q, kv = RS.attn_inputs(*case)
        out[case] = (q, kv, *RS.attn_ref(q, kv, *case))
    return out


@pytest.mark.parametrize("case", RS.ATTN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bar_passes_an_honest_split_key_kernel(attn_cases, case):
    q, kv, ref, bar = attn_cases[case]
    w = RS.worst(RS.emulate(q, kv, *case), ref, bar)
    print(f"latent attention bar, honest emulation {case}: worst ratio {w:.3f}")
    assert w < 1.0


def test_bar_catches_every_faulty_kernel_tenfold(attn_cases):
    """Every mutation is at least 10 x the bar on at least one case (a NaN counts as caught)."""
    for mut in MUTATIONS:
        ws = {}
        for case in RS.ATTN_CASES:
            q, kv, ref, bar = attn_cases[case]
            ws[case] = RS.worst(RS.emulate(q, kv, *case, **{mut: True}), ref, bar)
        print(f"latent attention bar, {mut}: " + ", ".join(f"{'x'.join(map(str, c))}: {w:.1f}" for c, w in ws.items()))
        assert max(ws.values()) >= 10.0, mut
        if mut == "no_factors":                    # wherever two waves hold keys
            assert all(w >= 10.0 for c, w in ws.items() if c[3] > RS.KEY_TILE)
        if mut == "padded_scale":                  # where the head dim is padded (80, 104); the honest kernel at 64; one key has no softmax
            assert all(w >= 10.0 for c, w in ws.items() if RS.padded(c[4]) != c[4] and c[3] > 1)
            assert all(w < 1.0 for c, w in ws.items() if RS.padded(c[4]) == c[4] or c[3] == 1)
        if mut == "no_latent_keys":
            assert all(w >= 10.0 for w in ws.values())


# ---------------------------------------------------------------------------------------------------------------- the loader
GEO = dict(E=160, dim=64, dim_head=32, heads=4, T=4, depth=2)


@pytest.mark.parametrize("which,layout", [("sd", "original"), ("sd", "nested"), ("xl", "original")])
def test_loader_reads_the_plus_layout_and_infers_every_dimension(which, layout):
    from rich_text_to_image_amd.ip_adapter import load_ip_adapter
    cfg = TINY_XL_CONFIG if which == "xl" else TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=3)
    ck, want, proj = RS.synthetic_plus_checkpoint(cfg, sd, **GEO, layout=layout)
    ad = load_ip_adapter(ck, cfg, dim_head=32)
    D = cfg["cross_attention_dim"]
    assert (ad["T"], ad["D"], ad["E"]) == (4, D, 160) and ad["image_proj"] == {}
    r = ad["resampler"]
    assert {k: r[k] for k in ("E", "dim", "D", "T", "depth", "heads", "dim_head", "inner", "ff")} == dict(
        E=160, dim=64, D=D, T=4, depth=2, heads=4, dim_head=32, inner=128, ff=256)
    assert set(r["weights"]) == set(proj) and all(torch.equal(r["weights"][k], proj[k]) for k in proj)
    assert set(ad["weights"]) == set(want) and all(torch.equal(ad["weights"][k], want[k]) for k in want)
    assert load_ip_adapter(ck, cfg)["resampler"]["heads"] == 2         # the default dim_head of 64: inner 128 = 2 heads


def test_loader_names_the_key_of_anything_unusable(tmp_path):
    from rich_text_to_image_amd.ip_adapter import load_ip_adapter
    cfg = TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=3)
    D = cfg["cross_attention_dim"]
    base = RS.synthetic_plus_checkpoint(cfg, sd, **GEO)[0]
    cases = [
        (lambda c: c.pop("image_proj.latents"), "image_proj.latents"),
        (lambda c: c.pop("image_proj.proj_in.bias"), "image_proj.proj_in.bias"),
        (lambda c: c.pop("image_proj.layers.1.0.to_kv.weight"), "image_proj.layers.1.0.to_kv.weight"),
        (lambda c: c.pop("image_proj.layers.0.1.3.weight"), "image_proj.layers.0.1.3.weight"),
        (lambda c: c.pop("image_proj.norm_out.weight"), "image_proj.norm_out.weight"),
        (lambda c: c.update({"image_proj.layers.0.0.to_v.weight": torch.zeros(128, 64)}), "image_proj.layers.0.0.to_v.weight"),
        (lambda c: c.update({"image_proj.pos_emb.weight": torch.zeros(4, 64)}), "image_proj.pos_emb.weight"),
        (lambda c: c.update({"image_proj.latents": torch.zeros(1, 17, 64)}), "image_proj.latents"),
        (lambda c: c.update({"image_proj.latents": torch.zeros(4, 64)}), "image_proj.latents"),
        (lambda c: c.update({"image_proj.layers.1.0.norm1.weight": torch.zeros(65)}), "image_proj.layers.1.0.norm1.weight"),
        (lambda c: c.update({"image_proj.layers.0.0.to_kv.weight": torch.zeros(128, 64)}), "image_proj.layers.0.0.to_kv.weight"),
        (lambda c: c.update({"image_proj.proj_out.weight": torch.zeros(D + 8, 64), "image_proj.proj_out.bias": torch.zeros(D + 8),
                             "image_proj.norm_out.weight": torch.zeros(D + 8), "image_proj.norm_out.bias": torch.zeros(D + 8)}), "image_proj.proj_out.weight"),
        (lambda c: c.pop("ip_adapter.1.to_k_ip.weight"), "ip_adapter.1.to_k_ip.weight"),
        (lambda c: c.update({"ip_adapter.99.to_k_ip.weight": torch.zeros(8, D)}), "ip_adapter.99.to_k_ip.weight"),
        (lambda c: c.update({"image_proj.proj.weight": torch.zeros(4 * D, 24)}), "Resampler"),          # both projections in one file
    ]
    for mutate, needle in cases:
        ck = dict(base)
        mutate(ck)
        with pytest.raises(ValueError) as e:
            load_ip_adapter(ck, cfg, dim_head=32)
        assert needle in str(e.value), (needle, str(e.value))
    with pytest.raises(ValueError) as e:                              # inner = 128 is no multiple of 48
        load_ip_adapter(dict(base), cfg, dim_head=48)
    assert "to_q.weight" in str(e.value) and "dim_head" in str(e.value)
    for bad in (0, 12, 136, 64.0):
        with pytest.raises(ValueError) as e:
            load_ip_adapter(dict(base), cfg, dim_head=bad)
        assert "dim_head" in str(e.value)
    torch.save(base, tmp_path / "plus.bin")                           # from a file, as the command line reads it
    assert load_ip_adapter(str(tmp_path / "plus.bin"), cfg, dim_head=32)["resampler"]["depth"] == 2


def test_a_linear_checkpoint_loads_as_before():
    """The dict of a linear checkpoint: the keys and values it had before the plus layout was read (no resampler= key); its mixed-file
    refusal still says Resampler."""
    from rich_text_to_image_amd.ip_adapter import load_ip_adapter
    cfg = TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=3)
    ck, want = R.synthetic_checkpoint(cfg, sd, T=4, E=24)
    ad = load_ip_adapter(ck, cfg)
    assert set(ad) == {"weights", "image_proj", "T", "D", "E"} and (ad["T"], ad["D"], ad["E"]) == (4, cfg["cross_attention_dim"], 24)
    assert set(ad["image_proj"]) == {"proj.weight", "proj.bias", "norm.weight", "norm.bias"}
    assert all(torch.equal(ad["image_proj"][k], ck["image_proj." + k].float()) for k in ad["image_proj"])
    assert set(ad["weights"]) == set(want) and all(torch.equal(ad["weights"][k], want[k]) for k in want)
    with pytest.raises(ValueError) as e:
        load_ip_adapter(dict(ck, **{"image_proj.latents": torch.zeros(1, 16, 8)}), cfg)
    assert "Resampler" in str(e.value)


# ---------------------------------------------------------------------------------------------------------------- entries and tool
def test_check_entry_under_a_plus_adapter():
    from rich_text_to_image_amd.ip_adapter import check_entry, load_ip_adapter
    cfg = TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=3)
    D = cfg["cross_attention_dim"]
    plus = load_ip_adapter(RS.synthetic_plus_checkpoint(cfg, sd, **GEO)[0], cfg, dim_head=32)
    e = check_entry(dict(hidden=torch.ones(17, 160), scale=0.5), "t", plus)
    assert e["scale"] == 0.5 and tuple(e["hidden"].shape) == (17, 160) and e["hidden"].dtype == torch.float32
    assert tuple(check_entry(dict(tokens=torch.ones(3, D)), "t", plus)["tokens"].shape) == (3, D)
    with pytest.raises(ValueError) as err:
        check_entry(dict(embeds=torch.ones(160)), "t", plus)
    assert "plus" in str(err.value) and "embeds" in str(err.value)
    for bad in (dict(hidden=torch.ones(17, 161)), dict(hidden=torch.ones(160)), dict(hidden=torch.ones(653, 160)), dict(hidden=torch.ones(0, 160)),
                dict(hidden=torch.full((2, 160), float("nan"))), dict(hidden=torch.ones(2, 160), tokens=torch.ones(2, D)),
                dict(hidden=torch.ones(2, 160), weight=1.0), dict(), dict(image="x.png")):
        with pytest.raises(ValueError):
            check_entry(bad, "t", plus)
    assert tuple(check_entry(dict(hidden=torch.ones(652, 160)), "t", plus)["hidden"].shape) == (652, 160)       # 652 + 4 latents = the limit
    # a linear adapter: hidden stays an unknown key, with the message it always had
    linear = load_ip_adapter(R.synthetic_checkpoint(cfg, sd, T=4, E=24)[0], cfg)
    with pytest.raises(ValueError) as err:
        check_entry(dict(hidden=torch.ones(17, 24)), "t", linear)
    assert str(err.value) == "t: expected exactly one of embeds= / tokens= / image= and an optional scale=, got keys ['hidden']"
    assert tuple(check_entry(dict(embeds=torch.ones(24)), "t", linear)["embeds"].shape) == (24,)


def test_facade_and_embedding_files_under_a_plus_adapter(tmp_path):
    """set_image_prompts takes hidden=; an encoder is matched by its hidden_size; a [t <= T, D] file is tokens, any other matrix hidden
    states."""
    import numpy as np
    from rich_text_to_image_amd.ip_adapter import apply_specs, image_prompts_from_specs
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    cfg = TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=3)
    D = cfg["cross_attention_dim"]
    m = RegionDiffusion(0, unet_state_dict=sd, config=cfg)
    m.load_ip_adapter(RS.synthetic_plus_checkpoint(cfg, sd, **GEO)[0], dim_head=32)
    assert m.ip_adapter["resampler"]["heads"] == 4
    m.set_image_prompts(base=dict(hidden=torch.ones(10, 160)), regions={0: dict(tokens=torch.ones(2, D))})
    assert "hidden" in m.image_prompts["base"] and "tokens" in m.image_prompts["regions"][0]
    with pytest.raises(ValueError):
        m.set_image_prompts(base=dict(embeds=torch.ones(160)))
    np.save(tmp_path / "tok.npy", np.ones((3, D), np.float32))
    np.save(tmp_path / "hid.npy", np.ones((1, 10, 160), np.float32))
    np.save(tmp_path / "emb.npy", np.ones((160,), np.float32))
    apply_specs(m, image_prompts_from_specs([f"{tmp_path / 'tok.npy'}:base", f"{tmp_path / 'hid.npy'}:0:0.5"]))
    assert tuple(m.image_prompts["base"]["tokens"].shape) == (3, D)
    assert tuple(m.image_prompts["regions"][0]["hidden"].shape) == (10, 160) and m.image_prompts["regions"][0]["scale"] == 0.5
    with pytest.raises(ValueError) as err:
        apply_specs(m, image_prompts_from_specs([f"{tmp_path / 'emb.npy'}"]))
    assert "plus" in str(err.value)

    class Enc:                                      # what check_entry reads of an image encoder
        S, projection_dim, hidden_size = 56, 160, 48
        def __call__(self, *a, **k):
            raise AssertionError("nothing is encoded before a sampling call")
    m.load_image_encoder(Enc())
    arr = np.zeros((60, 70, 3), np.uint8)
    with pytest.raises(ValueError) as err:          # projection_dim fits, hidden_size does not: the Resampler takes hidden states
        m.set_image_prompts(base=dict(image=arr))
    assert "hidden_size" in str(err.value) and "48" in str(err.value) and "160" in str(err.value)
    Enc.hidden_size, Enc.projection_dim = 160, 48
    m.set_image_prompts(base=dict(image=arr))
    assert tuple(m.image_prompts["base"]["image"].shape) == (56, 56, 3)


def test_make_image_encoder_writes_a_plus_adapter_the_loader_accepts(tmp_path):
    from rich_text_to_image_amd.clip_vision_encoder import LazyImageEncoder
    from rich_text_to_image_amd.ip_adapter import load_ip_adapter
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_image_encoder.py"), str(tmp_path / "enc"), "--adapter", str(tmp_path / "plus.bin"),
                        "--plus"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    ad = load_ip_adapter(str(tmp_path / "plus.bin"), TINY_SD_CONFIG)
    enc = LazyImageEncoder(str(tmp_path / "enc"))
    assert ad["resampler"]["dim_head"] == 64 and ad["E"] == enc.hidden_size == 160 and ad["T"] == 4


# ---------------------------------------------------------------------------------------------------------------- the chain
@pytest.mark.parametrize("geo", RS.GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_bf16_chain_against_the_fp64_resampler(geo):
    """Weights N(0, 1 / fan_in) x 1.  The chain of resampler.py with its bf16 roundings stays within the project's bar for this arithmetic
    class (relative L2 2e-2, test_encoder_matches_transformers'); the chain without the latents among the keys, and the one with the k and v
    halves of to_kv exchanged, are at least three bars away."""
    E, dim, dim_head, heads, T, depth, D, N, B = geo
    w = RS.random_resampler(E, dim, dim_head, heads, T, depth, D, seed=1)
    h = RS.hidden_inputs(B, N, E, seed=2)
    ref = RS.resampler_ref(w, h, dim_head)
    assert tuple(ref.shape) == (B, T, D)
    e_ok = RS.rel_l2(RS.resampler_emulate(w, h, dim_head), ref)
    e_lat = RS.rel_l2(RS.resampler_emulate(w, h, dim_head, no_latent_keys=True), ref)
    e_swap = RS.rel_l2(RS.resampler_emulate(w, h, dim_head, swap_kv=True), ref)
    print(f"Resampler chain {geo}: bf16 emulation {e_ok:.3e}, latents left out of the keys {e_lat:.3e}, k / v halves swapped {e_swap:.3e}")
    assert e_ok < 2e-2
    assert e_lat >= 6e-2 and e_swap >= 6e-2
