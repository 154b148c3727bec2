"""Pins the oracle against the UNMODIFIED reference UNet: its state_dict layout and one forward, as stored in
tests/golden/reference_unet.pt by oracle/make_reference_unet_golden.py (which runs the reference module itself)."""
import os

import pytest
import torch

from oracle.shapes import weight_shapes
from oracle.unet import SD15_CONFIG, SDXL_CONFIG, TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_unet.pt")


@pytest.fixture(scope="module")
def ref():
    return torch.load(GOLDEN)


@pytest.mark.parametrize("cfg,xl", [(TINY_XL_CONFIG, True), (TINY_SD_CONFIG, False)], ids=["tiny_xl", "tiny_sd"])
def test_state_dict_layout_and_forward(ref, cfg, xl, request):
    name = request.node.callspec.id
    rsd = ref["layout"][name]
    shapes = weight_shapes(cfg)
    assert set(shapes) == set(rsd)
    assert all(tuple(rsd[k]) == tuple(v) for k, v in shapes.items())
    f = ref["forward"][name]
    assert (f["added"] is not None) == xl
    sd = random_state_dict(cfg, seed=1)
    with torch.no_grad():
        y = OracleUNet(cfg, sd).forward(f["x"], f["t"], f["ctx"], f["added"])
    assert (f["reference_sample"] - y).abs().max().item() < 1e-5


@pytest.mark.parametrize("cfg", [SD15_CONFIG, SDXL_CONFIG], ids=["sd15", "sdxl"])
def test_full_size_layout_on_meta_device(ref, cfg, request):
    rsd = ref["layout"][request.node.callspec.id]
    shapes = weight_shapes(cfg)
    assert set(shapes) == set(rsd)
    assert all(tuple(rsd[k]) == tuple(v) for k, v in shapes.items())
