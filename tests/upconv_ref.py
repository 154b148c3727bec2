"""Plain-torch restatement of the sub-pixel form of Upsample2D's convolution (csrc/elementwise.hip pack_up2_kernel, csrc/gemm16.hip MODE =
A_CONV3_UP2): conv3x3(nearest-2x(x)) at output pixel (2y + a, 2x + b) = a 2x2 convolution of x over the pixels (y + a - 1 + r, x + b - 1 + c)."""
import torch
import torch.nn.functional as F

# 3x3 taps that fall on row r (column c) of the 2x2 window, per parity a (b) of the output row (column)
TAPS = {0: ((0,), (1, 2)), 1: ((0, 1), (2,))}


def phase_pack_ref(w):
    """w [Cout, Cin, 3, 3] -> [phase 2a + b][Cout][(tap 2r + c) * Cin + ci], summed ky-major / kx-minor in w's dtype."""
    Cout, Cin = w.shape[:2]
    out = torch.zeros(4, Cout, 4, Cin, dtype=w.dtype)
    for a in (0, 1):
        for b in (0, 1):
            for r in (0, 1):
                for c in (0, 1):
                    acc = torch.zeros(Cout, Cin, dtype=w.dtype)
                    for ky in TAPS[a][r]:
                        for kx in TAPS[b][c]:
                            acc = acc + w[:, :, ky, kx]
                    out[2 * a + b, :, 2 * r + c] = acc
    return out.reshape(4, Cout, 4 * Cin)


def upconv_phases(x, pack, bias=None):
    """x [B, Cin, H, W], pack from phase_pack_ref -> [B, Cout, 2H, 2W]: the four phase convolutions, zero padding on the low-resolution map."""
    B, Cin, H, W = x.shape
    Cout = pack.shape[1]
    out = torch.zeros(B, Cout, 2 * H, 2 * W, dtype=x.dtype)
    xp = F.pad(x, (1, 1, 1, 1))
    for a in (0, 1):
        for b in (0, 1):
            k = pack[2 * a + b].reshape(Cout, 2, 2, Cin).permute(0, 3, 1, 2)          # [Cout, Cin, r, c]
            # window rows y + a - 1 + r of x = rows y + a + r of the padded map
            y = F.conv2d(xp[:, :, a:a + H + 1, b:b + W + 1], k)
            out[:, :, a::2, b::2] = y
    return out if bias is None else out + bias.view(1, -1, 1, 1)
