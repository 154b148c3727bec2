"""VAE encoder on the GPU (RegionDiffusion.encode_imgs, rd.py:238-246): the stride-2 bottom / right-padded convolution of the GEMM
(A_CONV3_S2P0) at kernel level, the encoder's moments against the fp32 restatement (tests/vae_encoder_ref.py; parity against
diffusers unpinned), the logvar clamp, the posterior sample, and the façade's encode_imgs."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from hiputil import bf, gemm  # noqa: E402
from oracle.vae import SD_VAE_CONFIG, TINY_VAE_CONFIG, random_vae_state_dict  # noqa: E402
from vae_encoder_ref import OracleVAEEncoder, random_vae_encoder_state_dict  # noqa: E402

DEV = "cuda:0"
A_CONV3_S2P0, EPI_F32 = 4, 1


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


# ------------------------------------------------------------------------------------------------ kernel level
# (Cin, Cout, Hin, Win).  Split-K (gemm.hip splitk_slices: <= 96 tiles of 128 x 128, >= 8 K tiles) takes the 24x40 / 64x64 maps of
# 128+ channels; 16x16 x 8 channels (2 K tiles) and 256x256 x 128 (128 tiles) run as one launch.
@pytest.mark.parametrize("cin,cout,hin,win", [(8, 128, 16, 16), (128, 128, 24, 40), (256, 256, 24, 40), (512, 512, 64, 64),
                                              (128, 128, 256, 256)])
def test_conv_s2p0_matches_torch(cin, cout, hin, win):
    g = torch.Generator().manual_seed(cin + hin)
    x = torch.randn(1, cin, hin, win, generator=g).bfloat16().float()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / (3 * cin ** 0.5)).bfloat16().float()
    b = torch.randn(cout, generator=g) * 0.1
    out = gemm(bf(x.permute(0, 2, 3, 1)), bf(w.permute(0, 2, 3, 1).reshape(cout, -1)), bias=b.to(DEV), epi=EPI_F32, mode=A_CONV3_S2P0,
               conv=(hin // 2, win // 2))
    got = out.cpu().reshape(1, hin // 2, win // 2, cout).permute(0, 3, 1, 2)
    ref = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, b, stride=2)
    sym = F.conv2d(x, w, b, stride=2, padding=1)                     # the same map one pixel shifted
    r, r_sym = rel_l2(got, ref), rel_l2(got, sym)
    print(f"s2p0 conv {cin}->{cout} {hin}x{win}: rel-L2 {r:.2e} (vs symmetric padding {r_sym:.2e})")
    assert got.shape == ref.shape and r < 1e-4
    assert r_sym > 0.1


def test_conv_s2p0_rejects_odd_or_wrong_geometry():
    x = bf(torch.randn(1, 15, 16, 8))
    w = bf(torch.randn(8, 72))
    with pytest.raises(RuntimeError):
        gemm(x, w, epi=EPI_F32, mode=A_CONV3_S2P0, conv=(8, 8))      # Hin odd
    x = bf(torch.randn(1, 16, 16, 8))
    with pytest.raises(RuntimeError):
        gemm(x, w, epi=EPI_F32, mode=A_CONV3_S2P0, conv=(9, 8))      # Hout != Hin / 2


# ------------------------------------------------------------------------------------------------ encoder vs the restatement
def _encoder(cfg, lat_h, lat_w, sd, precise):
    from rich_text_to_image_amd.engine import VaeEncoder
    return VaeEncoder(cfg, lat_h, lat_w, device=0, state_dict=sd, precise=precise)


def _check_moments(enc, oracle, x, bar, tag):
    with torch.no_grad():
        ref = oracle.moments(x)
    d = enc.encode(x.to(DEV)).latent_dist
    rm, rv = rel_l2(d.mean, ref[:, :4]), rel_l2(d.logvar, ref[:, 4:])
    print(f"{tag}: mean rel-L2 {rm:.3e}, logvar rel-L2 {rv:.3e}")
    assert d.mean.shape == ref[:, :4].shape
    assert rm < bar and rv < bar


@pytest.mark.parametrize("precise,bar", [(False, 2e-2), (True, 3e-4)], ids=["single", "precise"])
def test_tiny_encoder_matches_oracle(precise, bar):
    sd = random_vae_encoder_state_dict(TINY_VAE_CONFIG, seed=1)
    enc, o = _encoder(TINY_VAE_CONFIG, 16, 24, sd, precise), OracleVAEEncoder(TINY_VAE_CONFIG, sd)
    g = torch.Generator().manual_seed(0)
    for hw in [(64, 64), (128, 192)]:
        _check_moments(enc, o, torch.rand(2, 3, *hw, generator=g) * 2 - 1, bar, f"tiny {hw} precise={precise}")
    enc.close()


@pytest.mark.parametrize("precise,bar", [(False, 2e-2), (True, 3e-4)], ids=["single", "precise"])
def test_sd_encoder_512_matches_oracle(precise, bar):
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = random_vae_encoder_state_dict(SD_VAE_CONFIG, seed=2)
    enc, o = _encoder(SD_VAE_CONFIG, 64, 64, sd, precise), OracleVAEEncoder(SD_VAE_CONFIG, sd)
    x = torch.rand(1, 3, 512, 512, generator=torch.Generator().manual_seed(1)) * 2 - 1
    _check_moments(enc, o, x, bar, f"SD 512^2 precise={precise}")
    enc.close()


def test_sdxl_encoder_1024_precise_matches_oracle():
    from rich_text_to_image_amd.engine import SDXL_VAE_CONFIG
    torch.set_num_threads(min(16, torch.get_num_threads()))
    sd = random_vae_encoder_state_dict(SDXL_VAE_CONFIG, seed=3)
    enc, o = _encoder(SDXL_VAE_CONFIG, 128, 128, sd, True), OracleVAEEncoder(SDXL_VAE_CONFIG, sd)
    x = torch.rand(1, 3, 1024, 1024, generator=torch.Generator().manual_seed(2)) * 2 - 1
    _check_moments(enc, o, x, 3e-4, "SDXL 1024^2 precise")
    enc.close()


def test_logvar_clamp_bounds_are_exact():
    sd = random_vae_encoder_state_dict(TINY_VAE_CONFIG, seed=3)
    sd["quant_conv.weight"] = sd["quant_conv.weight"].clone()
    sd["quant_conv.weight"][4:] *= 100
    enc, o = _encoder(TINY_VAE_CONFIG, 8, 8, sd, False), OracleVAEEncoder(TINY_VAE_CONFIG, sd)
    x = torch.rand(1, 3, 64, 64, generator=torch.Generator().manual_seed(0)) * 2 - 1
    lv = enc.encode(x.to(DEV)).latent_dist.logvar.cpu()
    with torch.no_grad():
        ref = o.moments(x)[:, 4:]
    lo, hi = ref == -30.0, ref == 20.0
    assert lo.any() and hi.any()
    assert (lv[lo] == -30.0).all() and (lv[hi] == 20.0).all()
    assert lv.min().item() == -30.0 and lv.max().item() == 20.0


# ------------------------------------------------------------------------------------------------ posterior
@pytest.fixture(scope="module")
def tiny_enc():
    sd = random_vae_encoder_state_dict(TINY_VAE_CONFIG, seed=4)
    enc = _encoder(TINY_VAE_CONFIG, 16, 16, sd, False)
    yield enc, sd
    enc.close()


def test_posterior_sample_follows_torch_rng(tiny_enc):
    enc, _ = tiny_enc
    x = (torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(5)) * 2 - 1).to(DEV)
    out = enc.encode(x)
    d = out.latent_dist
    m1 = d.moments.clone()
    assert torch.equal(enc.encode(x).latent_dist.moments, m1)                     # same input, same bits
    assert d.mode() is d.mean and torch.equal(d.mean, m1[:, :4]) and torch.equal(d.logvar, m1[:, 4:])

    def ref(eps, scale=1.0):
        return (d.mean + torch.exp(0.5 * d.logvar) * eps) * scale
    torch.manual_seed(11)
    s = d.sample()
    torch.manual_seed(11)
    eps = torch.randn(d.mean.shape, device=DEV, dtype=torch.float32)
    torch.testing.assert_close(s, ref(eps), rtol=2e-6, atol=1e-6)
    torch.manual_seed(11)
    torch.testing.assert_close(d.sample(scale=0.18215), ref(eps, 0.18215), rtol=2e-6, atol=1e-6)
    for gdev in ("cpu", DEV):                                                    # an explicit generator, on either device
        s = d.sample(generator=torch.Generator(device=gdev).manual_seed(7))
        eps = torch.randn(d.mean.shape, generator=torch.Generator(device=gdev).manual_seed(7), device=gdev).to(DEV)
        torch.testing.assert_close(s, ref(eps), rtol=2e-6, atol=1e-6)
    assert not torch.equal(d.sample(generator=torch.Generator(device=DEV).manual_seed(8)), s)


def test_roles_are_checked(tiny_enc):
    from rich_text_to_image_amd.engine import RtError, VaeDecoder, _ptr
    enc, _ = tiny_enc
    z, img_out = torch.zeros(4, 8, 8, device=DEV), torch.zeros(3, 64, 64, device=DEV)
    assert enc.lib.rt_vae_decode(enc.h, _ptr(z), 8, 8, 0, _ptr(img_out)) == -3                 # decode on an encoder handle
    dec = VaeDecoder(TINY_VAE_CONFIG, 8, 8, device=0, state_dict=random_vae_state_dict(TINY_VAE_CONFIG, seed=0))
    img, mom = torch.zeros(3, 64, 64, device=DEV), torch.zeros(8, 8, 8, device=DEV)
    assert dec.lib.rt_vae_encode(dec.h, _ptr(img), 64, 64, C.c_float(1.0), C.c_float(0.0), _ptr(mom)) == -3
    dec.close()
    with pytest.raises(RtError) as e:                                             # larger than the plan (16 x 16 latent)
        enc.encode(torch.zeros(1, 3, 136, 128, device=DEV))
    assert e.value.code == -1


# ------------------------------------------------------------------------------------------------ façade
def _write_checkpoint(root):
    """The synthetic diffusers-layout directory of test_checkpoint_gpu with a vae/ that holds decoder AND encoder weights."""
    import os
    from safetensors.torch import save_file
    from test_checkpoint_gpu import _write_dir
    _write_dir(root)
    sd = dict(random_vae_state_dict(TINY_VAE_CONFIG, seed=2))
    esd = random_vae_encoder_state_dict(TINY_VAE_CONFIG, seed=6)
    sd.update(esd)
    save_file({k: v.contiguous() for k, v in sd.items()}, os.path.join(root, "vae", "diffusion_pytorch_model.safetensors"))
    return esd


def _oracle_latents(esd, imgs, seed):
    with torch.no_grad():
        m = OracleVAEEncoder(TINY_VAE_CONFIG, esd).moments(2 * imgs - 1)
    torch.manual_seed(seed)
    eps = torch.randn(m[:, :4].shape, device=DEV).cpu()
    return (m[:, :4] + torch.exp(0.5 * m[:, 4:]) * eps) * 0.18215


def test_encode_imgs_from_checkpoint(tmp_path):
    from rich_text_to_image_amd.checkpoint import load_pipeline
    from rich_text_to_image_amd.engine import RtError
    esd = _write_checkpoint(str(tmp_path))
    m = load_pipeline(str(tmp_path), "SD", device=0, latent_hw=(64, 64))
    imgs = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(9))
    torch.manual_seed(21)
    lat = m.encode_imgs(imgs)
    assert lat.shape == (2, 4, 16, 16)
    r = rel_l2(lat, _oracle_latents(esd, imgs, 21))
    print(f"encode_imgs (lazy encoder from vae/): rel-L2 {r:.3e}")
    assert r < 2e-2
    first = m._lazy_encoder[0]
    big = torch.rand(1, 3, 192, 128, generator=torch.Generator().manual_seed(10))           # larger than the first plan: rebuilt
    torch.manual_seed(22)
    lat = m.encode_imgs(big)
    assert lat.shape == (1, 4, 24, 16) and m._lazy_encoder[0] is not first
    assert rel_l2(lat, _oracle_latents(esd, big, 22)) < 2e-2
    with pytest.raises(RtError):
        m.encode_imgs(torch.rand(1, 3, 100, 128))


def test_encode_imgs_with_vae_encoder_keyword():
    from oracle.unet import TINY_SD_CONFIG, random_state_dict
    from rich_text_to_image_amd.engine import RtError
    from rich_text_to_image_amd.region_diffusion import RegionDiffusion
    esd = random_vae_encoder_state_dict(TINY_VAE_CONFIG, seed=6)
    enc = _encoder(TINY_VAE_CONFIG, 16, 16, esd, False)
    m = RegionDiffusion(0, unet_state_dict=random_state_dict(TINY_SD_CONFIG, seed=1), config=TINY_SD_CONFIG, vae_encoder=enc)
    imgs = torch.rand(2, 3, 128, 128, generator=torch.Generator().manual_seed(9))
    torch.manual_seed(21)
    lat = m.encode_imgs(imgs)
    assert lat.shape == (2, 4, 16, 16) and rel_l2(lat, _oracle_latents(esd, imgs, 21)) < 2e-2
    with pytest.raises(RtError):
        m.encode_imgs(torch.rand(1, 3, 128, 100))
    enc.close()
