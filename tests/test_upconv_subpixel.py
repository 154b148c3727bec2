"""The identity behind the phase form of Upsample2D's convolution, in fp64 on the CPU (no GPU): four 2x2 convolutions of the low-resolution
map with summed taps = conv3x3(nearest-2x(x)) with zero padding, borders included; and what rounding the SUMS once costs against rounding the
nine taps (the engine's 3x3 pack) - the reason the phase pack is derived from the source tensor and not from the bf16 arena."""
import pytest
import torch
import torch.nn.functional as F

from upconv_ref import phase_pack_ref, upconv_phases


def _rel(a, b):
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


@pytest.mark.parametrize("B,Cin,Cout,H,W", [(2, 64, 96, 8, 8), (1, 24, 40, 5, 9), (1, 8, 8, 1, 1)])
def test_four_phase_convolutions_equal_the_upsampled_3x3_convolution(B, Cin, Cout, H, W):
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64) * (9 * Cin) ** -0.5
    bias = torch.randn(Cout, generator=g, dtype=torch.float64)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w, bias, padding=1)
    got = upconv_phases(x, phase_pack_ref(w), bias)
    assert (got - ref).abs().max().item() < 1e-12


def test_rounding_the_sums_once_is_no_worse_than_rounding_nine_taps():
    g = torch.Generator().manual_seed(4)
    B, Cin, Cout, H, W = 1, 256, 128, 12, 12
    x = torch.randn(B, Cin, H, W, generator=g).to(torch.bfloat16).double()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) * (9 * Cin) ** -0.5)
    ref = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w.double(), padding=1)
    nine = F.conv2d(F.interpolate(x, scale_factor=2.0, mode="nearest"), w.to(torch.bfloat16).double(), padding=1)
    once = upconv_phases(x, phase_pack_ref(w).to(torch.bfloat16).double())
    twice = upconv_phases(x, phase_pack_ref(w.to(torch.bfloat16).float()).to(torch.bfloat16).double())       # from the rounded 3x3 pack: NOT what the engine does
    e9, e1, e2 = _rel(nine, ref), _rel(once, ref), _rel(twice, ref)
    print(f"weight-rounding rel-L2: nine taps {e9:.3e}, sums rounded once {e1:.3e} ({e1 / e9:.2f} x), sums of rounded taps {e2:.3e} ({e2 / e9:.2f} x)")
    assert e1 <= 1.1 * e9
    assert e2 > 1.2 * e9          # sqrt(17 / 9) = 1.37 expected
