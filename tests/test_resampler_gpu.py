"""The Resampler of the IP-Adapter "plus" checkpoints on the GPU (csrc/resampler.hip; rich_text_to_image_amd/resampler.py):
rt_op_latent_attention against the fp64 restatement of tests/resampler_ref.py under its derived bar and under the memory contract, its
refusals, HipResampler against the fp64 Resampler, a plus adapter end to end on the tiny SD UNet (a picture, hidden states, a picture per
region), the bits of a linear adapter's run, and the command line."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

import clip_vision_ref as V
import ip_adapter_ref as R
import memguard as G
import resampler_ref as RS
from hiputil import DEV, chk
from oracle.unet import TINY_SD_CONFIG, random_state_dict
from rich_text_to_image_amd.engine import _ptr, load_library

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "resampler_linear_bits.json")
RT_E_INVALID = -1


# ---------------------------------------------------------------------------------------------------------------- the kernel
def _latent(q, kv, B, H, Nq, Nk, d, out, ldq=None, ldkv=None, ldo=None, q_off=0):
    lib = load_library()
    return lib.rt_op_latent_attention(C.c_void_p(q.data_ptr() + q_off), ldq if ldq is not None else q.stride(0), _ptr(kv),
                                      C.c_void_p(kv.data_ptr() + H * d * kv.element_size()), ldkv if ldkv is not None else kv.stride(0), _ptr(out),
                                      ldo if ldo is not None else out.stride(0), B, H, Nq, Nk, d, C.c_float(d ** -0.5), None)


@pytest.mark.parametrize("case", RS.ATTN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_latent_attention_matches_the_fp64_restatement_inside_its_windows(case):
    """q [B Nq, ldq = H d + 8] and kv [B Nk, ldkv = 2 H d + 16] (k | v per row) are different buffers with different leading dimensions,
    each in a NaN-poisoned window (padding columns and guards); the output sits in a guarded window with ldo > H d: guards intact, every
    interior element written and finite, worst |got - ref| / bar < 1, and a second launch gives the same bits."""
    B, H, Nq, Nk, d = case
    q, kv = RS.attn_inputs(*case)
    ref, bar = RS.attn_ref(q, kv, *case)
    q_p = G.poisoned(q.to(DEV), H * d + 8)
    kv_p = G.poisoned(kv.to(DEV), 2 * H * d + 16)
    big, out = G.guarded((B * Nq, H * d), torch.bfloat16, H * d + 8, device=DEV)
    chk(_latent(q_p, kv_p, *case, out))
    torch.cuda.synchronize()
    assert G.intact(big, out), G.damage(big, out)
    assert G.unwritten(out) == 0
    w = RS.worst(out.cpu(), ref, bar)
    print(f"rt_op_latent_attention {case}: worst |got - ref| / bar = {w:.3f}")
    assert w < 1.0
    big2, out2 = G.guarded((B * Nq, H * d), torch.bfloat16, H * d + 8, device=DEV)
    chk(_latent(q_p, kv_p, *case, out2))
    torch.cuda.synchronize()
    assert G.intact(big2, out2) and torch.equal(out2, out)


def test_latent_attention_refusals():
    """Nq 0 and 17, Nk 0 and 657, d 12 and 136, a bad ldq / ldkv / ldo and a misaligned pointer: RT_E_INVALID, and nothing is written."""
    lib = load_library()
    H, d = 2, 64
    good = dict(Nq=16, Nk=273, d=d, ldq=H * d, ldkv=2 * H * d, ldo=H * d, q_off=0)
    bad = [dict(Nq=0), dict(Nq=17), dict(Nk=0), dict(Nk=657), dict(d=12), dict(d=136), dict(ldq=H * d + 4), dict(ldkv=2 * H * d + 4), dict(ldo=H * d + 2),
           dict(ldq=H * d - 8), dict(q_off=8)]
    q = torch.zeros(32, 2 * 136 + 8, device=DEV, dtype=torch.bfloat16)
    kv = torch.zeros(660, 4 * 136 + 8, device=DEV, dtype=torch.bfloat16)
    out = torch.zeros(32, 2 * 136 + 8, device=DEV, dtype=torch.bfloat16)
    for b in bad:
        a = dict(good, **b)
        rc = _latent(q, kv, 1, H, a["Nq"], a["Nk"], a["d"], out, ldq=a["ldq"], ldkv=a["ldkv"], ldo=a["ldo"], q_off=a["q_off"])
        assert rc == RT_E_INVALID, (b, rc)
        assert "latent attention" in lib.rt_op_last_error().decode(), b
    torch.cuda.synchronize()
    assert not bool(out.any())
    a = good                                                            # the same call with nothing wrong runs
    chk(_latent(q, kv, 1, H, a["Nq"], a["Nk"], a["d"], out, ldq=a["ldq"], ldkv=a["ldkv"], ldo=a["ldo"]))
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------- the Resampler
@pytest.mark.parametrize("geo", RS.GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_hip_resampler_matches_the_fp64_resampler(geo):
    """Weights N(0, 1 / fan_in) x 1 (tests/test_resampler.py says why not x 3), bar 2e-2 relative L2 - test_encoder_matches_transformers'
    bar for this arithmetic class.  Two images in one call give the bits of two calls of one image."""
    from rich_text_to_image_amd.resampler import HipResampler, check_resampler
    E, dim, dim_head, heads, T, depth, D, N, B = geo
    w = RS.random_resampler(E, dim, dim_head, heads, T, depth, D, seed=1)
    r = check_resampler(w, dim_head)
    assert (r["E"], r["dim"], r["D"], r["T"], r["depth"], r["heads"]) == (E, dim, D, T, depth, heads)
    rs = HipResampler(r, device=0)
    assert len(rs.parameter_tensors()) == 7 + 11 * depth
    h = RS.hidden_inputs(2, N, E, seed=2)
    got = rs(h[:B])
    ref = RS.resampler_ref(w, h[:B], dim_head)
    e = RS.rel_l2(got, ref)
    print(f"HipResampler {geo}: rel-L2 against the fp64 Resampler = {e:.3e}")
    assert tuple(got.shape) == (B, T, D) and got.dtype == torch.float32 and bool(torch.isfinite(got).all())
    assert e < 2e-2
    both = got if B == 2 else rs(h)
    assert torch.equal(both[0], rs(h[:1])[0]) and torch.equal(both[1], rs(h[1:])[0])


# ---------------------------------------------------------------------------------------------------------------- end to end
PLUS = dict(E=160, dim=64, dim_head=64, heads=2, T=4, depth=2)            # E = the hidden size of V.ENCODER_CASES[0]


def _linear_adapter_digest():
    """SHA-256 of the latents of two plain steps of the tiny SD UNet under a LINEAR adapter with an image embedding: the run that must
    keep its bits when no plus adapter is loaded."""
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    cfg = TINY_SD_CONFIG
    g = torch.Generator().manual_seed(77)
    hw = 32
    sd = random_state_dict(cfg, seed=12)
    emb = torch.randn(2, 77, cfg["cross_attention_dim"], generator=g)
    lat = torch.randn(1, 4, hw, hw, generator=g)
    e = torch.randn(24, generator=g)
    m = RegionDiffusion(0, unet_state_dict=sd, config=cfg)
    m.load_ip_adapter(R.synthetic_checkpoint(cfg, sd, T=4, E=24, seed=5)[0])
    m.set_image_prompts(base=dict(embeds=e, scale=0.8))
    out = m.plain_latents(emb, 8 * hw, 8 * hw, 2, 7.5, lat.clone()).cpu()
    return hashlib.sha256(out.float().contiguous().numpy().tobytes()).hexdigest()


def test_a_linear_adapter_keeps_the_bits_it_had():
    """With no plus adapter loaded nothing new is allocated or launched: the digest of a linear-adapter run equals the one the same call
    gave BEFORE the Resampler existed (tests/golden/resampler_linear_bits.json, recorded on an MI355X from the parent commit)."""
    digest = _linear_adapter_digest()
    with open(GOLDEN) as f:
        want = json.load(f)["tiny_sd_linear_adapter_two_plain_steps"]
    print(f"linear adapter, two plain steps: sha256 {digest}")
    assert digest == want


def test_a_plus_adapter_end_to_end():
    """tiny SD, a tiny random encoder, a synthetic plus adapter whose E is the encoder's hidden size: image=arr gives, bit for bit, the
    latents of tokens=resampler(enc(preprocess(arr), output_hidden_states=True).hidden_states[-2]) and of hidden= those hidden states,
    differs from the run without an image; a different picture per region works in the rich pass; after unload_ip_adapter() a linear
    adapter still works and the pipeline without one equals a fresh one."""
    from rich_text_to_image_amd.clip_vision_encoder import HipCLIPVisionEncoder, preprocess
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    from rich_text_to_image_amd.resampler import HipResampler
    cfg = TINY_SD_CONFIG
    case = V.ENCODER_CASES[0]
    g = torch.Generator().manual_seed(31)
    hw, R_ = 32, 3
    sd = random_state_dict(cfg, seed=12)
    emb = torch.randn(R_ + 1, 77, cfg["cross_attention_dim"], generator=g)
    lat = torch.randn(1, 4, hw, hw, generator=g)
    masks = torch.softmax(torch.randn(R_, 1, hw, hw, generator=g) * 2, 0).repeat(1, 4, 1, 1)
    ck = RS.synthetic_plus_checkpoint(cfg, sd, **PLUS, seed=5)[0]
    ref = V.random_vision_model(case)
    arr, arr2 = V.synthetic_image(90, 120, seed=3), V.synthetic_image(64, 64, seed=8)

    def plain(m):
        return m.plain_latents(emb[[0, R_]], 8 * hw, 8 * hw, 2, 7.5, lat.clone()).cpu()

    def rich(m):
        return m.produce_latents(emb, height=8 * hw, width=8 * hw, num_inference_steps=2, guidance_scale=7.5, latents=lat.clone(),
                                 inject_selfattn=0.5, inject_background=0.4).cpu()

    def pipeline():
        m = RegionDiffusion(0, unet_state_dict=sd, config=cfg)
        m.masks = [masks[r:r + 1] for r in range(R_)]
        return m
    m0 = pipeline()
    never, never_r = plain(m0), rich(m0)
    m = pipeline()
    m.load_ip_adapter(ck)
    enc = HipCLIPVisionEncoder(ref.state_dict(), ref.config, device=0)
    m.load_image_encoder(enc)
    m.set_image_prompts(base=dict(image=arr))
    by_image = plain(m)
    hs = enc(torch.from_numpy(preprocess(arr, enc.S).copy())[None], output_hidden_states=True).hidden_states[-2]
    assert tuple(hs.shape) == (1, 17, 160)
    assert torch.equal(m.image_prompts["base"]["_hidden"], hs[0].cpu())    # encoded once, cached next to the tokens
    tokens = HipResampler(m.ip_adapter["resampler"], device=0)(hs)[0]
    assert tuple(tokens.shape) == (4, cfg["cross_attention_dim"]) and torch.equal(m.image_prompts["base"]["_tokens"], tokens.cpu())
    m.set_image_prompts(base=dict(tokens=tokens))
    assert torch.equal(plain(m), by_image)
    m.set_image_prompts(base=dict(hidden=hs[0]))
    assert torch.equal(plain(m), by_image)
    assert RS.rel_l2(by_image, never) > 1e-3
    # a picture per region, and one for the base prompt
    m.set_image_prompts(base=dict(image=arr, scale=0.7), regions={0: dict(image=arr2), 1: dict(image=arr, scale=0.6)})
    on_r = rich(m)
    assert bool(torch.isfinite(on_r).all()) and RS.rel_l2(on_r, never_r) > 1e-3
    m.set_image_prompts(base=dict(image=arr, scale=0.7), regions={0: dict(image=arr), 1: dict(image=arr, scale=0.6)})
    assert not torch.equal(rich(m), on_r)                                # region 0's picture matters
    # unload, then a linear adapter on the same pipeline
    m.unload_ip_adapter()
    assert torch.equal(plain(m), never)
    m.load_ip_adapter(R.synthetic_checkpoint(cfg, sd, T=4, E=case[7], seed=5)[0])
    m.set_image_prompts(base=dict(image=arr))                            # the pooled embedding again: E = projection_dim
    lin = plain(m)
    assert "_embeds" in m.image_prompts["base"] and "_hidden" not in m.image_prompts["base"]
    assert RS.rel_l2(lin, never) > 1e-3 and not torch.equal(lin, by_image)
    with pytest.raises(ValueError):
        m.set_image_prompts(base=dict(hidden=hs[0]))
    m.unload_ip_adapter()
    assert torch.equal(plain(m), never)


def test_sample_cli_runs_a_plus_adapter_from_an_image_file(tmp_path):
    """python -m rich_text_to_image_amd.sample --ip_adapter plus.bin --image_encoder DIR --ip_images a.png:0 on a synthetic checkpoint, a
    synthetic plus adapter and a randomly initialised encoder directory: the picture is read from disk, an image comes out, and the rich
    pass differs from the run without it."""
    from PIL import Image
    from safetensors.torch import save_file
    from rich_text_to_image_amd import sample
    from test_checkpoint_gpu import _write_dir
    _write_dir(str(tmp_path / "ckpt"))
    case = V.ENCODER_CASES[0]
    ref = V.random_vision_model(case)
    os.makedirs(tmp_path / "enc")
    with open(tmp_path / "enc" / "config.json", "w") as f:
        json.dump(dict(V.vision_config(case), model_type="clip_vision_model"), f)
    save_file({k: v.contiguous() for k, v in ref.state_dict().items()}, str(tmp_path / "enc" / "model.safetensors"))
    ck = RS.synthetic_plus_checkpoint(TINY_SD_CONFIG, random_state_dict(TINY_SD_CONFIG, seed=1), **PLUS)[0]
    torch.save(ck, tmp_path / "plus.bin")
    Image.fromarray(V.synthetic_image(90, 120, seed=3)).save(tmp_path / "a.png")
    js = json.dumps({"ops": [{"insert": "a "}, {"attributes": {"link": "a wooden fence covered in snow"}, "insert": "fence"},
                             {"insert": " under a night sky\n"}]})
    common = ["--load_path", str(tmp_path / "ckpt"), "--model", "SD", "--rich_text_json", js, "--sample_steps", "12", "--seed", "3", "--num_segments", "4",
              "--inject_selfattn", "0.2"]
    plain0, rich0 = sample.main(common + ["--run_dir", str(tmp_path / "out0")])
    plain, rich = sample.main(common + ["--run_dir", str(tmp_path / "out"), "--ip_adapter", str(tmp_path / "plus.bin"), "--image_encoder", str(tmp_path / "enc"),
                                        "--ip_images", f"{tmp_path / 'a.png'}:0"])
    assert plain.shape == rich.shape == (1, 512, 512, 3)
    assert os.path.exists(tmp_path / "out" / "seed3_plain.jpg") and os.path.exists(tmp_path / "out" / "seed3_rich.jpg")
    assert (rich != rich0).any()
