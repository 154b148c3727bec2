"""The UNet module by module: the engine's trunk tensor behind every traceable module (rt_unet_forward_trace: conv_in, every resnet,
every Transformer2DModel with its residual, every down / up sampler convolution, conv_out) against the CPU fp32 oracle's tensor at the
same place (OracleUNet ctl["trace"]), from ONE oracle forward per case.

The end-to-end tests see one number, the rel-L2 of the final eps (bound 1.5e-2).  Here every module gets that number, printed as a table
in execution order: an error that enters at one module shows as a step at its row.

Bound per module: the project's forward bound 1.5e-2 (tests/test_engine_gpu.py) - the arithmetic is the same at every depth (bf16
operands, fp32 accumulation, fp16 trunk) and the final output is the deepest point.  No module needed a bound of its own.

Measured on the MI355X, as the test prints it (rel-L2 per module, execution order).  The error enters at conv_in with the bf16 rounding of
the two operands (2.4e-3), grows by 3e-4 to 1.4e-3 per module down to the up blocks' first up-sampler (largest value anywhere: 1.217e-2,
SD-v1.5 up_blocks.0.upsamplers.0.conv) and FALLS again through the last up blocks, where the skip tensors of the shallow levels, which
carry little error, are concatenated in.  No row stands out as a step:
  tiny_xl_128 (128x128, t = 701):
    conv_in                            2.446e-03
    down_blocks.0.resnets.0            3.125e-03
    down_blocks.0.resnets.1            3.534e-03
    down_blocks.0.downsamplers.0.conv  4.272e-03
    down_blocks.1.resnets.0            5.866e-03
    down_blocks.1.attentions.0         6.202e-03
    down_blocks.1.resnets.1            6.745e-03
    down_blocks.1.attentions.1         6.949e-03
    down_blocks.1.downsamplers.0.conv  7.252e-03
    down_blocks.2.resnets.0            8.434e-03
    down_blocks.2.attentions.0         8.754e-03
    down_blocks.2.resnets.1            9.359e-03
    down_blocks.2.attentions.1         9.620e-03
    mid_block.resnets.0                9.748e-03
    mid_block.attentions.0             1.021e-02
    mid_block.resnets.1                1.046e-02
    up_blocks.0.resnets.0              1.149e-02
    up_blocks.0.attentions.0           1.177e-02
    up_blocks.0.resnets.1              1.184e-02
    up_blocks.0.attentions.1           1.157e-02
    up_blocks.0.resnets.2              1.066e-02
    up_blocks.0.attentions.2           1.041e-02
    up_blocks.0.upsamplers.0.conv      1.084e-02
    up_blocks.1.resnets.0              9.890e-03
    up_blocks.1.attentions.0           9.725e-03
    up_blocks.1.resnets.1              9.483e-03
    up_blocks.1.attentions.1           1.011e-02
    up_blocks.1.resnets.2              1.035e-02
    up_blocks.1.attentions.2           1.068e-02
    up_blocks.1.upsamplers.0.conv      1.137e-02
    up_blocks.2.resnets.0              9.918e-03
    up_blocks.2.resnets.1              8.359e-03
    up_blocks.2.resnets.2              7.077e-03
    conv_out                           7.605e-03
  tiny_sd_64 (64x64, t = 701):
    conv_in                            2.441e-03
    down_blocks.0.resnets.0            3.191e-03
    down_blocks.0.attentions.0         3.603e-03
    down_blocks.0.resnets.1            4.025e-03
    down_blocks.0.attentions.1         4.349e-03
    down_blocks.0.downsamplers.0.conv  5.007e-03
    down_blocks.1.resnets.0            6.190e-03
    down_blocks.1.attentions.0         6.451e-03
    down_blocks.1.resnets.1            6.966e-03
    down_blocks.1.attentions.1         6.930e-03
    down_blocks.1.downsamplers.0.conv  6.956e-03
    down_blocks.2.resnets.0            8.421e-03
    down_blocks.2.attentions.0         8.570e-03
    down_blocks.2.resnets.1            8.919e-03
    down_blocks.2.attentions.1         8.988e-03
    down_blocks.2.downsamplers.0.conv  9.361e-03
    down_blocks.3.resnets.0            9.974e-03
    down_blocks.3.resnets.1            1.029e-02
    mid_block.resnets.0                1.091e-02
    mid_block.attentions.0             1.087e-02
    mid_block.resnets.1                1.127e-02
    up_blocks.0.resnets.0              1.121e-02
    up_blocks.0.resnets.1              1.108e-02
    up_blocks.0.resnets.2              1.096e-02
    up_blocks.0.upsamplers.0.conv      1.132e-02
    up_blocks.1.resnets.0              1.060e-02
    up_blocks.1.attentions.0           1.097e-02
    up_blocks.1.resnets.1              1.101e-02
    up_blocks.1.attentions.1           1.129e-02
    up_blocks.1.resnets.2              1.112e-02
    up_blocks.1.attentions.2           1.137e-02
    up_blocks.1.upsamplers.0.conv      1.111e-02
    up_blocks.2.resnets.0              1.097e-02
    up_blocks.2.attentions.0           1.153e-02
    up_blocks.2.resnets.1              1.050e-02
    up_blocks.2.attentions.1           1.082e-02
    up_blocks.2.resnets.2              1.037e-02
    up_blocks.2.attentions.2           1.044e-02
    up_blocks.2.upsamplers.0.conv      1.065e-02
    up_blocks.3.resnets.0              9.435e-03
    up_blocks.3.attentions.0           9.761e-03
    up_blocks.3.resnets.1              7.916e-03
    up_blocks.3.attentions.1           8.071e-03
    up_blocks.3.resnets.2              7.297e-03
    up_blocks.3.attentions.2           7.695e-03
    conv_out                           8.252e-03
  tiny_sd_ragged_96 (96x96, t = 601):
    conv_in                            2.454e-03
    down_blocks.0.resnets.0            3.201e-03
    down_blocks.0.attentions.0         3.607e-03
    down_blocks.0.resnets.1            4.024e-03
    down_blocks.0.attentions.1         4.317e-03
    down_blocks.0.downsamplers.0.conv  4.950e-03
    down_blocks.1.resnets.0            6.212e-03
    down_blocks.1.attentions.0         6.419e-03
    down_blocks.1.resnets.1            6.833e-03
    down_blocks.1.attentions.1         6.792e-03
    down_blocks.1.downsamplers.0.conv  6.971e-03
    down_blocks.2.resnets.0            8.309e-03
    down_blocks.2.attentions.0         8.400e-03
    down_blocks.2.resnets.1            8.742e-03
    down_blocks.2.attentions.1         8.748e-03
    down_blocks.2.downsamplers.0.conv  9.127e-03
    down_blocks.3.resnets.0            9.796e-03
    down_blocks.3.resnets.1            1.019e-02
    mid_block.resnets.0                1.066e-02
    mid_block.attentions.0             1.070e-02
    mid_block.resnets.1                1.126e-02
    up_blocks.0.resnets.0              1.155e-02
    up_blocks.0.resnets.1              1.130e-02
    up_blocks.0.resnets.2              1.134e-02
    up_blocks.0.upsamplers.0.conv      1.176e-02
    up_blocks.1.resnets.0              1.042e-02
    up_blocks.1.attentions.0           1.077e-02
    up_blocks.1.resnets.1              1.129e-02
    up_blocks.1.attentions.1           1.152e-02
    up_blocks.1.resnets.2              1.141e-02
    up_blocks.1.attentions.2           1.166e-02
    up_blocks.1.upsamplers.0.conv      1.137e-02
    up_blocks.2.resnets.0              1.089e-02
    up_blocks.2.attentions.0           1.142e-02
    up_blocks.2.resnets.1              1.030e-02
    up_blocks.2.attentions.1           1.061e-02
    up_blocks.2.resnets.2              1.015e-02
    up_blocks.2.attentions.2           1.019e-02
    up_blocks.2.upsamplers.0.conv      1.047e-02
    up_blocks.3.resnets.0              9.561e-03
    up_blocks.3.attentions.0           9.806e-03
    up_blocks.3.resnets.1              7.948e-03
    up_blocks.3.attentions.1           8.134e-03
    up_blocks.3.resnets.2              7.338e-03
    up_blocks.3.attentions.2           7.722e-03
    conv_out                           8.231e-03
  sd15_64 (64x64, t = 801):
    conv_in                            2.404e-03
    down_blocks.0.resnets.0            3.216e-03
    down_blocks.0.attentions.0         3.571e-03
    down_blocks.0.resnets.1            3.991e-03
    down_blocks.0.attentions.1         4.225e-03
    down_blocks.0.downsamplers.0.conv  4.868e-03
    down_blocks.1.resnets.0            6.007e-03
    down_blocks.1.attentions.0         6.445e-03
    down_blocks.1.resnets.1            6.881e-03
    down_blocks.1.attentions.1         7.079e-03
    down_blocks.1.downsamplers.0.conv  7.460e-03
    down_blocks.2.resnets.0            8.474e-03
    down_blocks.2.attentions.0         8.685e-03
    down_blocks.2.resnets.1            9.128e-03
    down_blocks.2.attentions.1         9.217e-03
    down_blocks.2.downsamplers.0.conv  9.661e-03
    down_blocks.3.resnets.0            1.026e-02
    down_blocks.3.resnets.1            1.077e-02
    mid_block.resnets.0                1.120e-02
    mid_block.attentions.0             1.138e-02
    mid_block.resnets.1                1.166e-02
    up_blocks.0.resnets.0              1.192e-02
    up_blocks.0.resnets.1              1.184e-02
    up_blocks.0.resnets.2              1.197e-02
    up_blocks.0.upsamplers.0.conv      1.217e-02
    up_blocks.1.resnets.0              1.115e-02
    up_blocks.1.attentions.0           1.120e-02
    up_blocks.1.resnets.1              1.107e-02
    up_blocks.1.attentions.1           1.128e-02
    up_blocks.1.resnets.2              1.123e-02
    up_blocks.1.attentions.2           1.133e-02
    up_blocks.1.upsamplers.0.conv      1.175e-02
    up_blocks.2.resnets.0              1.071e-02
    up_blocks.2.attentions.0           1.092e-02
    up_blocks.2.resnets.1              9.759e-03
    up_blocks.2.attentions.1           9.957e-03
    up_blocks.2.resnets.2              9.672e-03
    up_blocks.2.attentions.2           9.887e-03
    up_blocks.2.upsamplers.0.conv      9.983e-03
    up_blocks.3.resnets.0              8.384e-03
    up_blocks.3.attentions.0           8.479e-03
    up_blocks.3.resnets.1              7.241e-03
    up_blocks.3.attentions.1           7.401e-03
    up_blocks.3.resnets.2              6.648e-03
    up_blocks.3.attentions.2           6.886e-03
    conv_out                           7.212e-03
  sdxl_128 (128x128, t = 801):
    conv_in                            2.416e-03
    down_blocks.0.resnets.0            3.205e-03
    down_blocks.0.resnets.1            3.732e-03
    down_blocks.0.downsamplers.0.conv  4.431e-03
    down_blocks.1.resnets.0            5.788e-03
    down_blocks.1.attentions.0         6.260e-03
    down_blocks.1.resnets.1            6.708e-03
    down_blocks.1.attentions.1         7.001e-03
    down_blocks.1.downsamplers.0.conv  7.409e-03
    down_blocks.2.resnets.0            8.395e-03
    down_blocks.2.attentions.0         8.456e-03
    down_blocks.2.resnets.1            8.740e-03
    down_blocks.2.attentions.1         8.751e-03
    mid_block.resnets.0                8.898e-03
    mid_block.attentions.0             9.063e-03
    mid_block.resnets.1                9.137e-03
    up_blocks.0.resnets.0              9.510e-03
    up_blocks.0.attentions.0           1.008e-02
    up_blocks.0.resnets.1              1.021e-02
    up_blocks.0.attentions.1           1.076e-02
    up_blocks.0.resnets.2              1.072e-02
    up_blocks.0.attentions.2           1.087e-02
    up_blocks.0.upsamplers.0.conv      1.151e-02
    up_blocks.1.resnets.0              1.082e-02
    up_blocks.1.attentions.0           1.136e-02
    up_blocks.1.resnets.1              1.011e-02
    up_blocks.1.attentions.1           1.047e-02
    up_blocks.1.resnets.2              1.018e-02
    up_blocks.1.attentions.2           1.007e-02
    up_blocks.1.upsamplers.0.conv      1.049e-02
    up_blocks.2.resnets.0              9.386e-03
    up_blocks.2.resnets.1              7.638e-03
    up_blocks.2.resnets.2              6.700e-03
    conv_out                           8.297e-03

Oracle time (16 threads): tiny configs 0.3 - 2 s, SD-v1.5 at 64x64 about 2.5 s, SDXL at 128x128 about 10 s (plus drawing its 2.6 G
random weights).  The engine runs one traced forward per module (30 - 50 forwards of a few ms to 60 ms).
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.unet import SD15_CONFIG, SDXL_CONFIG, TINY_SD_CONFIG, TINY_XL_CONFIG, INJECT_RESNET, OracleUNet, random_state_dict  # noqa: E402
import weight_influence_ref as W  # noqa: E402

DEV = "cuda:0"
BOUND = W.FORWARD_BOUND
OWN_BOUND = {}          # module -> (bound, reason): none needed so far

# name -> (config, weight seed, engine latent, forward latent (h, w), timestep): the sizes of tests/test_engine_gpu.py (128 / 64, and its
# ragged 96, whose deepest level has 12 x 12 = 144 tokens) and of tests/test_fullsize_gpu.py with its fixtures' seeds
CASES = {
    "tiny_xl_128": (TINY_XL_CONFIG, 11, 128, (128, 128), 701.0),
    "tiny_sd_64": (TINY_SD_CONFIG, 11, 64, (64, 64), 701.0),
    "tiny_sd_ragged_96": (TINY_SD_CONFIG, 11, 96, (96, 96), 601.0),
    "sd15_64": (SD15_CONFIG, 22, 64, (64, 64), 801.0),
    "sdxl_128": (SDXL_CONFIG, 21, 128, (128, 128), 801.0),
}


def _engine(cfg, sd, hw, max_streams=4, max_prompts=4):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(cfg, hw, hw, device=0, max_streams=max_streams, max_prompts=max_prompts)
    e.load_state_dict(sd)
    assert e.weights_missing()[0] == 0
    return e


def _set_prompts(eng, inp, scale=1.0):
    if inp["xl"]:
        eng.set_prompts((inp["emb"] * scale).to(DEV), inp["pooled"].to(DEV), inp["tid"])
    else:
        eng.set_prompts((inp["emb"] * scale).to(DEV))
    eng.set_fontsize(None, None)


@pytest.mark.parametrize("case", list(CASES))
def test_every_module_matches_the_oracle(case):
    cfg, seed, ehw, (h, w), t = CASES[case]
    sd = random_state_dict(cfg, seed=seed)
    inp = W.inputs(cfg, h, w, seed=31)
    added = {"text_embeds": inp["pooled"], "time_ids": inp["tid"]} if inp["xl"] else None
    ref = {}
    with torch.no_grad(), W.oracle_threads():
        ref_out = OracleUNet(cfg, sd).forward(inp["lat"], t, inp["emb"], added, ctl={"trace": ref})
    eng = _engine(cfg, sd, ehw, max_streams=1, max_prompts=1)
    del sd
    try:
        _set_prompts(eng, inp)
        x = inp["lat"].to(DEV)
        plain = eng.unet_forward(x, t, [0])
        mods = eng.trace_modules()
        assert [n for n, _, _ in mods] == list(ref)
        rows = []
        for name, ch, sh in mods:
            out, tr = eng.unet_forward(x, t, [0], trace=name)
            assert torch.equal(out, plain), f"{case}: tracing {name} changed the forward's output"
            assert tuple(tr.shape) == tuple(ref[name].shape) == (1, ch, h >> sh, w >> sh), (name, tuple(tr.shape), tuple(ref[name].shape))
            rows.append((name, W.rel_l2(tr, ref[name]), OWN_BOUND.get(name, (BOUND, ""))[0]))
        assert torch.equal(tr, plain)                                    # conv_out's tensor is the output itself
        print(f"\n{case}: rel-L2 of the engine's trunk against the oracle's behind every module ({h}x{w}, t = {t:.0f})")
        for name, r, b in rows:
            print(f"  {name:<34s} {r:.3e}{'' if r <= b else '   > ' + format(b, '.1e')}")
        print(f"  final output (untraced forward)    {W.rel_l2(plain, ref_out):.3e}")
        bad = [(n, r, b) for n, r, b in rows if not r <= b]
        assert not bad, bad
    finally:
        eng.close()


@pytest.fixture(scope="module")
def tiny_xl():
    sd = random_state_dict(TINY_XL_CONFIG, seed=11)
    eng = _engine(TINY_XL_CONFIG, sd, 64)
    yield TINY_XL_CONFIG, sd, eng
    eng.close()


def _mode_batch(cfg, hw):
    """The four streams of tests/test_engine_gpu.py's stream-mode forward: [uncond, base + font-size, text_ref, injected region]."""
    g = torch.Generator().manual_seed(123)
    emb = torch.randn(3, 77, cfg["cross_attention_dim"], generator=g)
    pooled = torch.randn(3, 32, generator=g)
    tid = torch.tensor([[hw * 8.0, hw * 8.0, 0, 0, hw * 8.0, hw * 8.0]])
    lat, lat_ref = torch.randn(1, 4, hw, hw, generator=g), torch.randn(1, 4, hw, hw, generator=g)
    return emb, pooled, tid, torch.cat([lat, lat, lat_ref, lat]), lat, lat_ref


def test_traced_forward_equals_untraced_bit_for_bit_under_every_mode_word(tiny_xl):
    """Font-size softmax, injected Q / K and the injected resnet feature, one word at a time and all together: `out` of a traced forward is
    rt_unet_forward's, whichever module is read - and the trace of the injected resnet is the oracle's for the injected stream too."""
    cfg, sd, eng = tiny_xl
    hw, t = 64, 701.0
    emb, pooled, tid, x, lat, lat_ref = _mode_batch(cfg, hw)
    eng.set_prompts(emb.to(DEV), pooled.to(DEV), tid)
    wp, fs = torch.tensor([3, 5]), torch.tensor([4.0, -2.0])
    eng.set_fontsize(wp, fs)
    x = x.to(DEV)
    modes = {
        "none": dict(),
        "fontsize": dict(fontsize=[0, 1, 0, 0]),
        "qk_src": dict(qk_src=[0, 1, 2, 2]),
        "res_src": dict(res_src=[-1, -1, -1, 2]),
        "in_scale": dict(in_scale=[1.0, 0.5, 1.0, 2.0]),
        "all": dict(fontsize=[0, 1, 0, 0], qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2], in_scale=[1.0, 0.5, 1.0, 2.0]),
    }
    names = [n for n, _, _ in eng.trace_modules()]
    probe = ["conv_in", "down_blocks.1.attentions.0", "mid_block.attentions.0", INJECT_RESNET, "up_blocks.1.upsamplers.0.conv", "conv_out"]
    assert set(probe) <= set(names)
    for mname, kw in modes.items():
        plain = eng.unet_forward(x, t, [0, 2, 2, 1], **kw)
        for name in probe:
            out, tr = eng.unet_forward(x, t, [0, 2, 2, 1], trace=name, **kw)
            assert torch.equal(out, plain), (mname, name)
            assert tr.shape[0] == 4 and torch.isfinite(tr).all()
        assert torch.equal(tr, plain)
        assert torch.equal(eng.unet_forward(x, t, [0, 2, 2, 1], **kw), plain), mname      # and a traced forward leaves nothing behind
    # the injected stream's resnet output against the oracle: shortcut(own input) + the text_ref stream's residual branch
    o = OracleUNet(cfg, sd)
    with torch.no_grad(), W.oracle_threads():
        cap = {}
        o.forward(lat_ref, t, emb[2:3], {"text_embeds": pooled[2:3], "time_ids": tid}, ctl={"capture": cap})
        inj = {k: v for k, v in cap.items() if k.endswith("attn1") or k == INJECT_RESNET}
        ref = {}
        o.forward(lat, t, emb[1:2], {"text_embeds": pooled[1:2], "time_ids": tid}, ctl={"inject": inj, "trace": ref, "trace_stop": INJECT_RESNET})
    _, tr = eng.unet_forward(x, t, [0, 2, 2, 1], trace=INJECT_RESNET, qk_src=[0, 1, 2, 2], res_src=[-1, -1, -1, 2])
    r = W.rel_l2(tr[3:4], ref[INJECT_RESNET])
    print(f"injected stream at {INJECT_RESNET}: rel-L2 {r:.3e}")
    assert r <= BOUND


def test_bad_trace_requests_are_errors_and_write_nothing(tiny_xl):
    from rich_text_to_image_amd.engine import RtError, _ptr
    cfg, sd, eng = tiny_xl
    hw, t = 64, 701.0
    emb, pooled, tid, x, _, _ = _mode_batch(cfg, hw)
    eng.set_prompts(emb.to(DEV), pooled.to(DEV), tid)
    eng.set_fontsize(None, None)
    x = x[:2].to(DEV).contiguous()
    for bad in ("conv_inn", "down_blocks.0", "down_blocks.0.resnets.0.conv1", "mid_block.attentions.0.transformer_blocks.0", ""):
        with pytest.raises(RtError):
            eng.unet_forward(x, t, [0, 1], trace=bad)
    shapes = {n: (c, s) for n, c, s in eng.trace_modules()}
    idx = (C.c_int * 2)(0, 1)
    for name in ("down_blocks.1.resnets.0", "conv_out"):
        ch, sh = shapes[name]
        need = 2 * ch * (hw >> sh) * (hw >> sh)
        tr = torch.full((need,), float("nan"), device=DEV)
        out = torch.full_like(x, float("nan"))
        rc = eng.lib.rt_unet_forward_trace(eng.h, _ptr(x), 2, hw, hw, C.c_float(t), None, idx, None, None, None, _ptr(out), name.encode(), _ptr(tr),
                                           C.c_longlong(need - 1))
        eng.synchronize()
        assert rc != 0 and "trace_cap_floats" in eng.lib.rt_last_error(eng.h).decode()
        assert torch.isnan(tr).all() and torch.isnan(out).all(), "a refused trace wrote something"
        rc = eng.lib.rt_unet_forward_trace(eng.h, _ptr(x), 2, hw, hw, C.c_float(t), None, idx, None, None, None, _ptr(out), name.encode(), _ptr(tr),
                                           C.c_longlong(need))
        eng.synchronize()
        assert rc == 0 and torch.isfinite(tr).all() and torch.isfinite(out).all()
    assert torch.equal(eng.unet_forward(x, t, [0, 1]), out)               # the engine is as usable as before
