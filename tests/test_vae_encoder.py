"""VAE encoder (RegionDiffusion.encode_imgs, rd.py:238-246) without a GPU: the weight table of an encoder handle created with
device -1 against the AutoencoderKL encoder + quant_conv shapes (tests/vae_encoder_ref.py), and the published parameter counts."""
import math

import pytest

from oracle.vae import SD_VAE_CONFIG, TINY_VAE_CONFIG, vae_decoder_shapes
from rich_text_to_image_amd.engine import SDXL_VAE_CONFIG, VaeDecoder, VaeEncoder
from vae_encoder_ref import vae_encoder_shapes


@pytest.mark.parametrize("cfg", [SD_VAE_CONFIG, TINY_VAE_CONFIG, SDXL_VAE_CONFIG], ids=["sd", "tiny", "sdxl"])
@pytest.mark.parametrize("precise", [False, True])
def test_encoder_weight_table_matches_shapes(cfg, precise):
    v = VaeEncoder(cfg, 64, 64, device=-1, precise=precise)
    table = v.weight_table()
    assert dict(table) == {k: tuple(s) for k, s in vae_encoder_shapes(cfg).items()}
    assert len(table) == len(vae_encoder_shapes(cfg))
    v.close()


def test_sd_encoder_parameter_count():
    v = VaeEncoder(SD_VAE_CONFIG, 64, 64, device=-1)
    shapes = v.weight_table()
    assert len(shapes) == 108
    assert sum(math.prod(s) for _, s in shapes) == 34_163_664


def test_encoder_plus_decoder_is_autoencoderkl():
    enc = VaeEncoder(SD_VAE_CONFIG, 64, 64, device=-1).weight_table()
    dec = VaeDecoder(SD_VAE_CONFIG, 64, 64, device=-1).weight_table()
    assert not {n for n, _ in enc} & {n for n, _ in dec}
    assert sum(math.prod(s) for _, s in dec) == sum(math.prod(s) for s in vae_decoder_shapes(SD_VAE_CONFIG).values()) == 49_490_199
    assert sum(math.prod(s) for _, s in enc + dec) == 83_653_863


def test_encoder_needs_four_latent_channels():
    with pytest.raises(ValueError):
        VaeEncoder(dict(TINY_VAE_CONFIG, latent_channels=16), 8, 8, device=-1)
