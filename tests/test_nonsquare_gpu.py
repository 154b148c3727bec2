"""GPU parity at the real architectures on latent grids whose height and width DIFFER (the product takes --height and --width
separately; every other end-to-end test steps a square latent, where a swapped (h, w) is a no-op and where rows per stream are
powers of two):

  * SDXL-base, latent  96x168 (768x1344):  rows per stream 16128 / 4032 / 1008 - the 1008-token level is ragged and outside the
    shared-softmax domain, no 3x3 convolution is patch-kernel eligible, LayerNorm-fold tiles straddle stream boundaries
  * SDXL-base, latent 128x96  (1024x768, portrait): rows 12288 / 3072 / 768 - 64x48 is patch-convolution eligible, 32x24 is not
  * SD-v1.5,   latent  64x96  (512x768):  tokens 6144 / 1536 / 384 / 96

Each: one batched rt_unet_forward with every stream mode word of a rich-text step against four oracle forwards, exactly as
tests/test_fullsize_gpu.py does on the square (same helpers, same bars: rel-L2 <= 1.5e-2 per stream), plus one injected rich-text
step (R = 4, inject_selfattn 0.5: seven streams, Euler) at SDXL 96x168 (latent UPDATE of both latent streams <= 3e-2 at CFG 5).
SDXL time_ids are original_size + crops_coords_top_left + target_size with (height, width), as the reference builds them.  The
masks are random and not symmetric under transposition.  Oracle outputs are committed under tests/golden/fullsize_oracle
(tests/oracle_cache.py --generate); the tests print where theirs came from.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import test_fullsize_gpu as fs  # noqa: E402   (helpers only: _build, _NoEngine, _stream_mode_forward, _masks, cached)
from oracle.schedulers import OracleEuler  # noqa: E402
from oracle.unet import SD15_CONFIG, SDXL_CONFIG, OracleUNet, random_state_dict  # noqa: E402
from oracle_cache import cached, weights_fingerprint  # noqa: E402

DEV, rel_l2 = fs.DEV, fs.rel_l2


@pytest.fixture(scope="module")
def sdxl_weights():
    sd = random_state_dict(SDXL_CONFIG, seed=21)
    o = OracleUNet(SDXL_CONFIG, sd)
    o.fingerprint = weights_fingerprint(sd)
    return sd, o


def _engine(cfg, sd, h, w):
    if fs.GENERATE:
        return fs._NoEngine()
    from rich_text_to_image_amd.engine import Engine
    eng = Engine(cfg, h, w, device=0, max_streams=8, max_prompts=8)
    eng.load_state_dict(sd)
    assert eng.weights_missing()[0] == 0
    return eng


@pytest.fixture(scope="module")
def sdxl_96x168(sdxl_weights):
    sd, o = sdxl_weights
    eng = _engine(SDXL_CONFIG, sd, 96, 168)
    yield eng, o
    eng.close()


def test_sdxl_landscape_96x168_stream_modes_match_oracle(sdxl_96x168):
    eng, o = sdxl_96x168
    res = fs._stream_mode_forward(eng, o, SDXL_CONFIG, 96, 168, True, 801.0, key="stream_modes_sdxl_96x168")
    for name, r in res.items():
        assert r < 1.5e-2, (name, r)


def test_sdxl_portrait_128x96_stream_modes_match_oracle(sdxl_weights):
    sd, o = sdxl_weights
    eng = _engine(SDXL_CONFIG, sd, 128, 96)
    try:
        res = fs._stream_mode_forward(eng, o, SDXL_CONFIG, 128, 96, True, 801.0, key="stream_modes_sdxl_128x96")
    finally:
        eng.close()
    for name, r in res.items():
        assert r < 1.5e-2, (name, r)


def test_sd15_landscape_64x96_stream_modes_match_oracle():
    eng, o = fs._build(SD15_CONFIG, 64, 96, 22, max_streams=8, max_prompts=8)
    try:
        res = fs._stream_mode_forward(eng, o, SD15_CONFIG, 64, 96, False, 701.0, key="stream_modes_sd15_64x96")
    finally:
        eng.close()
    for name, r in res.items():
        assert r < 1.5e-2, (name, r)


def test_sdxl_96x168_injected_rich_step_matches_oracle(sdxl_96x168):
    """test_sdxl_config3_rich_step_matches_oracle on the 768x1344 bucket: the injected first iteration of a 2-step Euler schedule
    (t = 501: seven streams, the three region streams with qk_src / res_src -> text_ref), both latent streams after the scheduler
    step, compared on the latent UPDATE."""
    from oracle.region_loop import rich_step_forwards
    eng, o = sdxl_96x168
    h, w, R, steps, gs, isa = 96, 168, 4, 2, 5.0, 0.5
    g = torch.Generator().manual_seed(41)
    emb = torch.randn(R + 1, 77, 2048, generator=g)
    pooled = torch.randn(R + 1, 1280, generator=g)
    original_size = target_size = (8.0 * h, 8.0 * w)                       # (height, width)
    tid = torch.tensor([list(original_size + (0.0, 0.0) + target_size)])
    m = fs._masks(R, h, w, g)
    assert rel_l2(m[:, :, :, :h], m[:, :, :, :h].transpose(2, 3)) > 0.1    # not symmetric under transposition
    masks = [m[r:r + 1] for r in range(R)]
    sched = OracleEuler(); sched.set_timesteps(steps)
    assert [float(t) > 500 for t in sched.timesteps] == [True, False]
    lat0 = torch.randn(1, 4, h, w, generator=g) * sched.init_noise_sigma
    tfd = {"word_pos": torch.tensor([5, 6]), "font_size": torch.tensor([20.0, 20.0])}
    eng.set_prompts(emb.to(DEV), pooled.to(DEV), tid)
    eng.set_masks(m.to(DEV))
    eng.set_fontsize(tfd["word_pos"], tfd["font_size"])
    eng.set_schedule(0, sched.timesteps.tolist(), sched.sigmas.tolist(), steps)
    eng.set_latents(lat0.to(DEV))
    eng.region_step(0, gs, isa, 0.0, xl=True, elide=False)
    got, got_ref = (t.cpu() for t in eng.read_latents(h, w, with_ref=True))

    def added_fn(k):
        k = k if k >= 0 else pooled.shape[0] + k
        return {"text_embeds": pooled[k:k + 1], "time_ids": tid}
    t = sched.timesteps[0]
    lat_in = sched.scale_model_input(lat0, t)
    (eu, et, eur, etr), hit = cached("sdxl_96x168_rich_step", o.fingerprint, [lat_in, emb, pooled, tid, m, tfd, float(t)],
                                     lambda: rich_step_forwards(o, lat_in, lat_in.clone(), t, emb, added_fn, masks, tfd, True, True))
    print("oracle outputs:", "tests/golden/fullsize_oracle" if hit else "computed live")
    out = sched.step(torch.cat([eu + gs * (et - eu), eur + gs * (etr - eur)]), t, torch.cat([lat0, lat0]))["prev_sample"]
    ref, ref_ref = torch.chunk(out, 2, dim=0)
    r, rr = rel_l2(got - lat0, ref - lat0), rel_l2(got_ref - lat0, ref_ref - lat0)
    print(f"SDXL @96x168, injected rich step (R=4, inject_selfattn=0.5): latent UPDATE rel-L2 {r:.3e} (reference stream {rr:.3e})")
    assert r < 3e-2 and rr < 3e-2


def test_full_width_vae_decode_and_guidance_gradient_at_32x48_match_oracle():
    """AutoencoderKL decoder at the real width (128-256-512-512) on a 32x48 latent (256x384 image), decode and the colour-guidance
    gradient against torch autograd through oracle/vae.py, live: a quarter of the work of the 64x64 case in tests/test_fullsize_gpu.py.
    Single bf16 pass, as the SD pipeline runs it: decode 2e-2, loss 2e-2, gradient and update 5e-2."""
    from oracle.vae import SD_VAE_CONFIG, OracleVAEDecoder, color_guidance_update, random_vae_state_dict
    from rich_text_to_image_amd.engine import VaeDecoder
    h, w = 32, 48
    sd = random_vae_state_dict(SD_VAE_CONFIG, seed=5)
    v = VaeDecoder(SD_VAE_CONFIG, h, w, device=0, state_dict=sd)
    o = OracleVAEDecoder(SD_VAE_CONFIG, sd)
    g = torch.Generator().manual_seed(2)
    z = torch.randn(1, 4, h, w, generator=g) * 3
    with torch.no_grad():
        ref = o.decode(z)
    out = v.decode(z.to(DEV))
    assert tuple(out.shape) == (1, 3, 8 * h, 8 * w)
    r = rel_l2(out, ref)
    print(f"full-width VAE decode {h}x{w} -> {8 * h}x{8 * w}: rel-L2 {r:.3e} (ref rms {ref.pow(2).mean().sqrt():.3f})")
    assert r < 2e-2
    lat, eps = torch.randn(1, 4, h, w, generator=g), torch.randn(1, 4, h, w, generator=g)
    masks = [(torch.rand(1, 1, 8 * h, 8 * w, generator=g) ** 2).repeat(1, 4, 1, 1) for _ in range(3)]      # n_color + 1 masks, as sample.py hands them over
    rgb = [torch.rand(1, 3, 1, 1, generator=g) for _ in range(2)]
    mall = torch.rand(1, 4, h, w, generator=g)
    alpha, sc, wgt = 0.37, SD_VAE_CONFIG["scaling_factor"], 0.5
    new_ref, grad_ref, loss_ref = color_guidance_update(o, lat, eps, alpha, sc, masks, rgb, wgt, mall)
    lat_g = lat.clone().to(DEV)
    loss, grad = v.color_guidance(lat_g, eps.to(DEV), alpha, h, w, masks, rgb, wgt, mall, want_grad=True)
    rg, ru = rel_l2(grad, grad_ref), rel_l2(lat_g.cpu() - lat, new_ref - lat)
    print(f"full-width colour guidance {h}x{w}: loss {loss:.4f} vs {loss_ref:.4f}; grad rel-L2 {rg:.3e}; update rel-L2 {ru:.3e}")
    assert abs(loss - loss_ref) < 2e-2 * abs(loss_ref)
    assert rg < 5e-2 and ru < 5e-2
    v.close()
