"""The CLIP vision encoder on the GPU (csrc/vision.hip; rich_text_to_image_amd/clip_vision_encoder.py): rt_op_bidir_attention against
the fp64 restatement of tests/clip_vision_ref.py under its derived bar and under the memory contract, the patch / class-token /
pre-LayerNorm front end against a direct fp64 computation, LayerNorm at the new widths, the whole encoder against transformers'
CLIPVisionModelWithProjection with the same weights, and a picture as an image prompt end to end."""
import ctypes as C
import hashlib
import json
import os

import pytest
import torch

import clip_vision_ref as V
import ip_adapter_ref as R
import memguard as G
from hiputil import DEV, chk, gemm, layernorm
from oracle.unet import TINY_SD_CONFIG, random_state_dict
from rich_text_to_image_amd.engine import RtError, _ptr, load_library

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "layernorm_bits.json")


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


# ---------------------------------------------------------------------------------------------------------------- attention
def _bidir(qkv, B, H, N, d, out, ld=None):
    lib = load_library()
    es = qkv.element_size()
    return lib.rt_op_bidir_attention(_ptr(qkv), C.c_void_p(qkv.data_ptr() + H * d * es), C.c_void_p(qkv.data_ptr() + 2 * H * d * es),
                                     ld or qkv.stride(0), _ptr(out), out.stride(0), B, H, N, d, C.c_float(d ** -0.5), None)


@pytest.mark.parametrize("case", V.ATTN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_bidir_attention_matches_the_fp64_restatement_inside_its_windows(case):
    """ld = 3 H d with q | k | v interleaved; the inputs sit in a NaN-poisoned window (padding columns and guards), the output in a
    guarded window with ldo > H d: guards intact, every interior element written and finite, worst |got - ref| / bar < 1."""
    B, H, N, d = case
    qkv = V.attn_inputs(*case)
    ref, bar = V.attn_ref(qkv, *case)
    qkv_p = G.poisoned(qkv.to(DEV), 3 * H * d + 8)
    big, out = G.guarded((B * N, H * d), torch.bfloat16, H * d + 8, device=DEV)
    chk(_bidir(qkv_p, *case, out))
    torch.cuda.synchronize()
    assert G.intact(big, out), G.damage(big, out)
    assert G.unwritten(out) == 0
    w = V.worst(out.cpu(), ref, bar)
    print(f"rt_op_bidir_attention {case}: worst |got - ref| / bar = {w:.3f}")
    assert w < 1.0
    # the exact layout the encoder passes (ld = 3 H d, ldo = H d): the same bits
    plain = torch.full((B * N, H * d), float("nan"), device=DEV, dtype=torch.bfloat16)
    chk(_bidir(qkv.to(DEV), *case, plain))
    torch.cuda.synchronize()
    assert torch.equal(plain, out)


def test_bidir_attention_refusals():
    """N = 641, d = 136 and d = 84 are refused on the host - RtError, as the encoder raises it -, and nothing is written."""
    lib = load_library()
    for N, d in ((641, 80), (257, 136), (257, 84)):
        qkv = torch.zeros(N, 6 * d, device=DEV, dtype=torch.bfloat16)
        out = torch.zeros(N, 2 * d, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(RtError) as e:
            rc = _bidir(qkv, 1, 2, N, d, out)
            if rc != 0:
                raise RtError(rc, lib.rt_op_last_error().decode())
        assert "bidir attention" in str(e.value)
        torch.cuda.synchronize()
        assert not bool(out.any())


# ---------------------------------------------------------------------------------------------------------------- front end
@pytest.mark.parametrize("S,p,B", [(56, 14, 2), (64, 32, 1)])
def test_front_end_matches_a_direct_fp64_computation(S, p, B):
    """patchify -> GEMM (the patch convolution) -> vit_embed against conv + class token + positions + LayerNorm in fp64; both kernels
    write into guarded windows; the padding columns of the patch rows are exactly zero."""
    lib = load_library()
    Cc, Gd = 160, S // p
    N, K, Kp = Gd * Gd + 1, 3 * p * p, (3 * p * p + 7) // 8 * 8
    g = torch.Generator().manual_seed(S + p)
    px = torch.randint(0, 256, (B, S, S, 3), generator=g, dtype=torch.uint8)
    conv_w = torch.randn(Cc, 3, p, p, generator=g) * K ** -0.5
    cls, pos = torch.randn(Cc, generator=g), torch.randn(N, Cc, generator=g) * 0.5
    gamma, beta = 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)
    mean, std = (C.c_float * 3)(*V.CLIP_MEAN), (C.c_float * 3)(*V.CLIP_STD)
    big_r, rows = G.guarded((B * Gd * Gd, Kp), torch.bfloat16, Kp, device=DEV)       # the operator writes dense rows
    px_p = G.poisoned(px.to(DEV))                                        # (every poisoned operand keeps a name: its allocation must outlive the launch)
    chk(lib.rt_op_patchify(_ptr(px_p), _ptr(rows), B, S, p, Kp, mean, std, None))
    torch.cuda.synchronize()
    assert G.intact(big_r, rows), G.damage(big_r, rows)
    assert G.unwritten(rows) == 0
    assert bool((rows[:, K:].view(torch.int16) == 0).all()), "padding columns of the patch rows are not exactly zero"
    want_rows = V.patch_rows_ref(px, p, Kp)
    err_rows = ((rows.double().cpu() - want_rows).abs() / (2.0 ** -8 * want_rows.abs() + 1e-6)).max().item()     # one bf16 rounding + the fp32 formula
    print(f"rt_op_patchify S={S} p={p}: worst |got - ref| / (2^-8 |ref| + 1e-6) = {err_rows:.3f}")
    assert err_rows < 1.0
    wp = torch.zeros(Cc, Kp)
    wp[:, :K] = conv_w.reshape(Cc, -1)
    patch = gemm(rows, wp.to(DEV).to(torch.bfloat16).contiguous(), None, epi=1)
    big_o, out = G.guarded((B * N, Cc), torch.float32, Cc, device=DEV)
    ops = [G.poisoned(t.to(DEV)) for t in (patch, cls, pos, gamma, beta)]
    chk(lib.rt_op_vit_embed(_ptr(ops[0]), Cc, _ptr(ops[1]), _ptr(ops[2]), _ptr(ops[3]), _ptr(ops[4]), _ptr(out), B, N, Cc, C.c_float(1e-5), None))
    torch.cuda.synchronize()
    assert G.intact(big_o, out), G.damage(big_o, out)
    assert G.unwritten(out) == 0
    ref = V.front_end_ref(px, p, conv_w, cls, pos, gamma, beta)
    # fp64 on the kernels' own bf16 operands: what is left is fp32 accumulation over K <= 3072 products and the fp32 LayerNorm - the
    # project's fp32-output bar (tests/test_kernels_gpu.py: F32_OUT)
    err = (out.double().cpu() - ref).abs()
    tol = 2e-3 + 2e-3 * ref.abs()
    print(f"front end S={S} p={p} B={B}: max |err| = {err.max().item():.3e}, rel-L2 = {rel_l2(out, ref):.3e}")
    assert bool((err <= tol).all())


# ---------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_case(rows, Cc):
    g = torch.Generator().manual_seed(70 + Cc)
    x = torch.randn(rows, Cc, generator=g) * 3 + 1
    return x, 1 + 0.1 * torch.randn(Cc, generator=g), 0.1 * torch.randn(Cc, generator=g)


@pytest.mark.parametrize("rows,Cc", [(257, 1664), (77, 2048), (5, 1544)])
def test_layernorm_at_the_new_widths(rows, Cc):
    """C in (1536, 2048]: the NP = 4 instantiation against fp64 within the bar of tests/test_kernels_gpu.py's test_layernorm
    (BF16_OUT: atol 2e-2, rtol 1.2e-2); 1544 = one 8-channel chunk into the fourth pass."""
    x, gamma, beta = _ln_case(rows, Cc)
    out = layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV))
    xd = x.double()
    ref = (xd - xd.mean(-1, keepdim=True)) / (xd.var(-1, unbiased=False, keepdim=True) + 1e-5).sqrt() * gamma.double() + beta.double()
    err = (out.double().cpu() - ref).abs()
    print(f"layernorm {rows}x{Cc}: max |err| = {err.max().item():.3e}")
    assert bool((err <= 2e-2 + 1.2e-2 * ref.abs()).all())


@pytest.mark.parametrize("rows,Cc", [(515, 1280), (96, 768)])
def test_layernorm_keeps_its_bits_at_the_old_widths(rows, Cc):
    """The 1280 route (layernorm40_kernel) and NP = 2 (768) against the SHA-256 of the output the same call gave BEFORE the NP = 4
    instantiation existed (tests/golden/layernorm_bits.json, recorded on an MI355X from the parent commit's library).  Accuracy at
    these widths is tests/test_kernels_gpu.py::test_layernorm's; this pins the bits."""
    x, gamma, beta = _ln_case(rows, Cc)
    out = layernorm(x.to(DEV), gamma.to(DEV), beta.to(DEV))
    digest = hashlib.sha256(out.cpu().view(torch.int16).numpy().tobytes()).hexdigest()
    with open(GOLDEN) as f:
        want = json.load(f)[f"{rows}x{Cc}"]
    print(f"layernorm {rows}x{Cc}: sha256 {digest}")
    assert digest == want


# ---------------------------------------------------------------------------------------------------------------- whole encoder
@pytest.mark.parametrize("case", V.ENCODER_CASES, ids=lambda c: f"C{c[0]}")
def test_encoder_matches_transformers(case):
    from rich_text_to_image_amd.clip_vision_encoder import HipCLIPVisionEncoder, preprocess
    hidden, heads, layers, mlp, act, image, patch, proj = case
    ref = V.random_vision_model(case)
    px = torch.stack([torch.from_numpy(preprocess(V.synthetic_image(300, 200, seed=s), image).copy()) for s in (1, 2)])
    pv = ((px.float() / 255.0 - torch.tensor(V.CLIP_MEAN)) / torch.tensor(V.CLIP_STD)).permute(0, 3, 1, 2).contiguous()
    with torch.no_grad():
        r = ref(pixel_values=pv, output_hidden_states=True)
    enc = HipCLIPVisionEncoder(ref.state_dict(), ref.config, device=0)
    o = enc(px, output_hidden_states=True)
    e_emb, e_pen = rel_l2(o.image_embeds, r.image_embeds), rel_l2(o.hidden_states[-2], r.hidden_states[-2])
    e_last, e_first = rel_l2(o.last_hidden_state, r.last_hidden_state), rel_l2(o.hidden_states[0], r.hidden_states[0])
    print(f"CLIP vision encoder C={hidden} H={heads} L={layers} {act} {image}/{patch}: image_embeds {e_emb:.3e}  hidden[-2] {e_pen:.3e}  "
          f"last {e_last:.3e}  (hidden[0] {e_first:.3e})")
    assert len(o.hidden_states) == layers + 1 and o.image_embeds.shape == r.image_embeds.shape == (2, proj)
    assert o.pooler_output.shape == (2, hidden) and o.last_hidden_state.shape == r.last_hidden_state.shape
    assert e_emb < 2e-2 and e_pen < 2e-2 and e_last < 2e-2              # bf16 operands, fp32 accumulation / residual stream
    assert len(enc.parameter_tensors()) == 8 + 12 * layers
    one = enc(px[:1])                                                   # an image alone (the GEMMs may tile another way: same bar, not same bits)
    assert one.hidden_states is None and rel_l2(one.image_embeds[0], r.image_embeds[0]) < 2e-2


# ---------------------------------------------------------------------------------------------------------------- end to end
def test_a_picture_as_image_prompt_end_to_end():
    """tiny SD, a synthetic adapter whose E is the encoder's projection_dim: image=arr gives, bit for bit, the latents of
    embeds=enc(preprocess(arr)).image_embeds[0] over two steps, differs from the run without an image, and a pipeline that loaded and
    unloaded an encoder equals a fresh one."""
    from rich_text_to_image_amd.clip_vision_encoder import HipCLIPVisionEncoder, preprocess
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    cfg = TINY_SD_CONFIG
    case = V.ENCODER_CASES[0]
    g = torch.Generator().manual_seed(31)
    hw = 32
    sd = random_state_dict(cfg, seed=12)
    emb = torch.randn(2, 77, cfg["cross_attention_dim"], generator=g)
    lat = torch.randn(1, 4, hw, hw, generator=g)
    ck, _ = R.synthetic_checkpoint(cfg, sd, T=4, E=case[7], seed=5)
    ref = V.random_vision_model(case)
    arr = V.synthetic_image(90, 120, seed=3)

    def plain(m):
        return m.plain_latents(emb, 8 * hw, 8 * hw, 2, 7.5, lat.clone()).cpu()
    never = plain(RegionDiffusion(0, unet_state_dict=sd, config=cfg))
    m = RegionDiffusion(0, unet_state_dict=sd, config=cfg)
    m.load_ip_adapter(ck)
    enc = HipCLIPVisionEncoder(ref.state_dict(), ref.config, device=0)
    m.load_image_encoder(enc)
    m.set_image_prompts(base=dict(image=arr))
    by_image = plain(m)
    e = enc(torch.from_numpy(preprocess(arr, enc.S).copy())[None]).image_embeds[0]
    assert torch.equal(m.image_prompts["base"]["_embeds"], e.cpu())       # encoded once, cached next to the tokens
    m.set_image_prompts(base=dict(embeds=e))
    by_embeds = plain(m)
    assert torch.equal(by_image, by_embeds)
    assert rel_l2(by_image, never) > 1e-3
    m.unload_image_encoder()
    m.unload_ip_adapter()
    assert torch.equal(plain(m), never)
    m2 = RegionDiffusion(0, unet_state_dict=sd, config=cfg)              # loaded and unloaded before anything ran
    m2.load_image_encoder(enc)
    m2.unload_image_encoder()
    assert torch.equal(plain(m2), never)


def test_sample_cli_runs_from_image_files(tmp_path):
    """python -m rich_text_to_image_amd.sample --ip_adapter A --image_encoder DIR --ip_images x.png:0 y.jpg:base:0.6 on a synthetic
    checkpoint, a synthetic adapter and a randomly initialised encoder directory: both pictures are read from disk, and both passes
    differ from the run without them."""
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
    ck, _ = R.synthetic_checkpoint(TINY_SD_CONFIG, random_state_dict(TINY_SD_CONFIG, seed=1), T=4, E=case[7])
    torch.save(ck, tmp_path / "ip.bin")
    Image.fromarray(V.synthetic_image(90, 120, seed=3)).save(tmp_path / "x.png")
    Image.fromarray(V.synthetic_image(200, 150, seed=4)).save(tmp_path / "y.jpg")
    js = json.dumps({"ops": [{"insert": "a "}, {"attributes": {"link": "a wooden fence covered in snow"}, "insert": "fence"},
                             {"insert": " under a night sky\n"}]})
    common = ["--load_path", str(tmp_path / "ckpt"), "--model", "SD", "--rich_text_json", js, "--sample_steps", "12", "--seed", "3", "--num_segments", "4",
              "--inject_selfattn", "0.2"]
    plain0, rich0 = sample.main(common + ["--run_dir", str(tmp_path / "out0")])
    plain, rich = sample.main(common + ["--run_dir", str(tmp_path / "out"), "--ip_adapter", str(tmp_path / "ip.bin"), "--image_encoder", str(tmp_path / "enc"),
                                        "--ip_images", f"{tmp_path / 'x.png'}:0", f"{tmp_path / 'y.jpg'}:base:0.6"])
    assert plain.shape == rich.shape == (1, 512, 512, 3)
    assert os.path.exists(tmp_path / "out" / "seed3_plain.jpg") and os.path.exists(tmp_path / "out" / "seed3_rich.jpg")
    assert (plain != plain0).any() and (rich != rich0).any()
