"""References for FreeU (csrc/freeu.hip, include/rtdiff.h: rt_set_freeu / rt_op_freeu).  Test infrastructure, plain torch / numpy.

  backbone_ref          x[:, :, c] * b for c < C1 // 2 (fp64; the kernel's result must equal (x.float() * b).half() bit for bit)
  skip_ref              the fp64 RESTATEMENT the tests pin: sk + (s - 1) / HW Re(sum_{(ky, kx) in {-1, 0}^2} X[ky, kx] e^{2 pi i (ky y / H + kx x / W)}),
                        X = fftn(sk), evaluated as four complex coefficients and the real part of their reconstruction.  Its keyword
                        arguments are the MUTATIONS tests/test_freeu.py proves the bar catches.
  fourier_filter_literal  the literal fp64 transcription of diffusers' fourier_filter(x, threshold, scale) ([memory] of
                        utils/torch_utils.py: fftn, fftshift, box mask, ifftshift, ifftn, .real) with torch.fft
  skip_fp32_numpy       the closed form in fp32 numpy, sums sequential over the tokens - what the simplest correct kernel would do
  bar                   the per-element bar of the fp16 result
  FreeUOracleUNet       oracle.unet.OracleUNet with the restatement in front of every resnet of up blocks 0 and 1

Layouts: the engine's tensors are token-major [B, H W, C]; the references work on maps [..., H, W] (to_maps / from_maps convert)."""
import functools
import math

import numpy as np
import torch

from oracle.unet import INJECT_RESNET, TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict

# The accumulation allowance of the bar, in units of |s - 1| max|sk| (max over the stream and channel).  MEASURED_FP32_DISTANCE is the
# largest distance of skip_fp32_numpy from skip_ref BEFORE the fp16 rounding, over the inputs of tests/test_freeu_gpu.py (op_inputs of
# every grid in OP_GRIDS, all seven streams; the two large grids on every 16th channel) at s in OP_S, measured on the CPU by
# tests/test_freeu.py::test_accumulation_allowance_is_the_measured_one, which re-measures it and fails when it no longer holds.  The
# largest value comes from the 64 x 64 grid at s = 0.9: 4096 sequential fp32 additions of values with a DC offset, and the rounding of the
# final fp32 addition, which weighs most in these units where |s - 1| is small.  (Written rounded up to two digits.)
# A = 4 x that: the GPU sums in another order (64 strided sequential series, then a tree), and a tree sum is within a small factor of a
# sequential one.  The number is never taken from what the kernel gives.
MEASURED_FP32_DISTANCE = 1.1e-6    # measured 1.005e-6 (64 x 64, s = 0.9)
ACCUMULATION_ALLOWANCE = 4.0 * MEASURED_FP32_DISTANCE

OP_GRIDS = ((2, 2), (2, 6), (3, 5), (4, 6), (8, 12), (32, 32), (64, 64))
LARGE_GRIDS = ((32, 32), (64, 64))
OP_CHANNELS_SMALL = ((64, 32),)
OP_CHANNELS_LARGE = ((64, 32), (1280, 1280), (1280, 640), (640, 320))
OP_STREAMS = (1, 3, 7)
OP_S = (0.2, 0.9, 1.5)


def to_maps(t, H, W):
    """[B, H W, C] -> [B, C, H, W]"""
    B, HW, C = t.shape
    assert HW == H * W
    return t.reshape(B, H, W, C).permute(0, 3, 1, 2)


def from_maps(m):
    """[B, C, H, W] -> [B, H W, C]"""
    B, C, H, W = m.shape
    return m.permute(0, 2, 3, 1).reshape(B, H * W, C)


@functools.lru_cache(maxsize=2)
def op_inputs(H, W):
    """The inputs of the op tests on an H x W grid: (hidden, skip), fp16 [7, H W, Cmax] on the CPU - normals with a per-channel offset
    (so that the DC term matters), a function of the grid alone; a case takes the leading [:B, :, :C] of each.  Cmax = 1280 on the two
    large grids (the only ones the wide channel pairs run on), 64 elsewhere."""
    cmax = 1280 if (H, W) in LARGE_GRIDS else 64
    g = torch.Generator().manual_seed(1000 * H + W)
    out = []
    for _ in range(2):
        off = 2.0 * torch.randn(cmax, generator=g)
        out.append((torch.randn(7, H * W, cmax, generator=g) + off).half())
    return tuple(out)


def backbone_ref(x, b, half=None):
    """x [B, HW, C1] -> fp64 [B, HW, C1]: channels < C1 // 2 times b.  (half: mutation - another channel count)"""
    out = x.double().clone()
    h = x.shape[-1] // 2 if half is None else half
    out[..., :h] *= b
    return out


def _phase(H, W, ky, kx, dev, swap_hw=False):
    y = torch.arange(H, dtype=torch.float64, device=dev)[:, None]
    x = torch.arange(W, dtype=torch.float64, device=dev)[None, :]
    if swap_hw:
        return 2.0 * math.pi * (ky * y / W + kx * x / H)
    return 2.0 * math.pi * (ky * y / H + kx * x / W)


def skip_ref(sk, s, *, kx_low=-1, count_conjugate=False, swap_hw=False, s_not_minus_one=False, no_dc=False):
    """sk [..., H, W] (any float type) -> fp64 [..., H, W].  Keyword arguments: mutations (all off = the contract).
      kx_low=+1         the bins {-1, 0} x {+1, 0}: the other diagonal (+1 on the x axis alone; flipping BOTH axes gives the conjugate
                        bins, which is invisible in the real part - and so is this one wherever H == 2 or W == 2, where -1 == +1)
      count_conjugate   every bin but DC counted together with its conjugate partner (the missing halving of taking .real)
      swap_hw           H and W swapped in the twiddles
      s_not_minus_one   the correction scaled by s instead of s - 1
      no_dc             the bin (0, 0) left out"""
    H, W = sk.shape[-2:]
    v = sk.double().reshape(-1, H * W)
    corr = torch.zeros_like(v)
    for ky in (-1, 0):
        for kx in (kx_low, 0):
            if no_dc and ky == 0 and kx == 0:
                continue
            ph = _phase(H, W, ky, kx, v.device, swap_hw).reshape(-1)
            er, ei = torch.cos(ph), torch.sin(ph)                      # e = exp(i ph)
            xr, xi = v @ er, -(v @ ei)                                 # X[ky, kx] = sum sk conj(e)
            term = xr[:, None] * er[None, :] - xi[:, None] * ei[None, :]      # Re(X e)
            corr += 2.0 * term if (count_conjugate and (ky, kx) != (0, 0)) else term
    f = s if s_not_minus_one else s - 1.0
    return (v + f * corr / (H * W)).reshape(sk.shape)


def fourier_filter_literal(x, threshold, scale):
    """diffusers' fourier_filter in fp64, step by step."""
    x = x.double()
    x_freq = torch.fft.fftn(x, dim=(-2, -1))
    x_freq = torch.fft.fftshift(x_freq, dim=(-2, -1))
    H, W = x.shape[-2:]
    mask = torch.ones(x.shape, dtype=torch.float64, device=x.device)
    crow, ccol = H // 2, W // 2
    mask[..., crow - threshold:crow + threshold, ccol - threshold:ccol + threshold] = scale
    x_freq = x_freq * mask
    x_freq = torch.fft.ifftshift(x_freq, dim=(-2, -1))
    return torch.fft.ifftn(x_freq, dim=(-2, -1)).real


def skip_fp32_numpy(sk, H, W, s):
    """sk fp16 numpy [N, H W] -> fp32 numpy [N, H W]: the closed form in fp32 before the rounding to fp16.  Twiddles correctly rounded
    to fp32 (as a precise sincospi gives them), the seven sums sequential over the tokens in fp32, the correction summed left to right."""
    f = np.float32
    v = sk.astype(f)
    N, HW = v.shape
    assert HW == H * W
    ty, tx = 2.0 * np.arange(H) / H, 2.0 * np.arange(W) / W
    cy, sy = np.cos(np.pi * ty).astype(f), np.sin(np.pi * ty).astype(f)
    cx, sx = np.cos(np.pi * tx).astype(f), np.sin(np.pi * tx).astype(f)
    for t_, c_, s_ in ((ty, cy, sy), (tx, cx, sx)):                   # exact where sincospi is exact: multiples of 1 / 2
        c_[np.isclose(t_ % 1.0, 0.5)] = 0.0
        s_[np.isclose(t_ % 1.0, 0.0)] = 0.0
    yy, xx = np.divmod(np.arange(HW), W)
    u = (cy[yy], sy[yy])
    w = (cx[xx], sx[xx])
    uw = ((u[0] * w[0] - u[1] * w[1]).astype(f), (u[1] * w[0] + u[0] * w[1]).astype(f))
    tw = [np.ones(HW, f), u[0], u[1], w[0], w[1], uw[0], uw[1]]
    acc = np.zeros((7, N), f)
    for t in range(HW):
        a = v[:, t]
        for k in range(7):
            acc[k] += a * tw[k][t]
    g = f((f(s) - f(1.0)) / f(HW))
    corr = np.zeros((N, HW), f)
    for k in range(7):
        corr += acc[k][:, None] * tw[k][None, :]
    return v + g * corr


def bar(ref, sk, s, allowance=None):
    """The bar of one fp16 output element: 2^-11 |ref| + 2^-25 (one fp16 rounding, with the subnormal floor) + A |s - 1| max|sk|, the
    maximum over the element's own (stream, channel) map.  ref, sk: [..., H, W]."""
    a = ACCUMULATION_ALLOWANCE if allowance is None else allowance
    mx = sk.double().abs().amax(dim=(-2, -1), keepdim=True)
    return 2.0 ** -11 * ref.double().abs() + 2.0 ** -25 + a * abs(s - 1.0) * mx


def round_bar(ref):
    """One fp16 rounding alone (the backbone half, which has no sums)."""
    return 2.0 ** -11 * ref.double().abs() + 2.0 ** -25


class FreeUOracleUNet(OracleUNet):
    """OracleUNet with FreeU: in front of every resnet of up blocks 0 and 1 the two channel slices of the concatenated input - hidden
    [:C1] and skip [C1:], C1 as oracle/shapes.py wires the up path - are rounded to fp16 (what the engine's trunk holds), run through
    the fp64 restatement and rounded to fp16 again."""

    def __init__(self, config, state_dict, s1, s2, b1, b2):
        super().__init__(config, state_dict)
        self.freeu = ((b1, s1), (b2, s2))

    def _hidden_channels(self, i, j):
        rboc = list(reversed(self.cfg["block_out_channels"]))
        return rboc[max(i - 1, 0)] if j == 0 else rboc[i]

    def _resnet(self, name, x, emb, ctl):
        parts = name.split(".")
        if parts[0] == "up_blocks" and parts[2] == "resnets" and int(parts[1]) < 2:
            i, j = int(parts[1]), int(parts[3])
            b, s = self.freeu[i]
            c1 = self._hidden_channels(i, j)
            hid, sk = x[:, :c1].half(), x[:, c1:].half()
            hid = backbone_ref(hid.permute(0, 2, 3, 1), b).permute(0, 3, 1, 2).half().float()
            sk = skip_ref(sk, s).half().float()
            x = torch.cat([hid, sk], dim=1)
        return super()._resnet(name, x, emb, ctl)


# ---------------------------------------------------------------------------------------------------------------- the forward tests
# the settings of the forward tests (tests/test_freeu_gpu.py) and of the discrimination test (tests/test_freeu.py).  The starting point (0.2, 0.1, 1.4, 1.6) moves tiny SD by 0.127
# only and (0.1, 0.05, 1.8, 2.0) by 0.151, a hair above the 0.15 tests/test_freeu.py::test_forward_settings_discriminate asks for: moved further from 1 until the
# plain oracle is 0.173 away on tiny SD (0.3 on tiny XL).  Chosen on the two CPU oracles alone.
FORWARD_FREEU = dict(s1=0.1, s2=0.05, b1=2.0, b2=2.4)
FORWARD_CASES = (("xl", TINY_XL_CONFIG, 16, 24), ("sd", TINY_SD_CONFIG, 32, 64))
FORWARD_BAR = 1.5e-2            # the project's forward bar (tests/test_engine_gpu.py)


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return ((a - b).pow(2).sum() / b.pow(2).sum()).sqrt().item()


def forward_case(which):
    """Inputs of the forward tests: tiny XL at 16 x 24 / tiny SD at 32 x 64 with the stream modes of
    test_batched_forward_with_stream_modes_matches_oracle (uncond, base + font size, text_ref, injected region)."""
    _, cfg, h, w = next(c for c in FORWARD_CASES if c[0] == which)
    xl = which == "xl"
    sd = random_state_dict(cfg, seed=11)
    g = torch.Generator().manual_seed(321)
    emb = torch.randn(3, 77, cfg["cross_attention_dim"], generator=g)
    pooled = torch.randn(3, 32, generator=g) if xl else None
    tid = torch.tensor([[h * 8.0, w * 8.0, 0, 0, h * 8.0, w * 8.0]]) if xl else None
    lat, lat_ref = torch.randn(1, 4, h, w, generator=g), torch.randn(1, 4, h, w, generator=g)
    return dict(cfg=cfg, sd=sd, xl=xl, h=h, w=w, emb=emb, pooled=pooled, tid=tid, lat=lat, lat_ref=lat_ref, t=701.0,
                wp=torch.tensor([3, 5]), fs=torch.tensor([4.0, -2.0]))


def oracle_streams(o, c):
    """The four streams on oracle `o`: [uncond, base + font size, text_ref, injected region]."""
    def added(k):
        return {"text_embeds": c["pooled"][k:k + 1], "time_ids": c["tid"]} if c["xl"] else None
    emb, t = c["emb"], c["t"]
    with torch.no_grad():
        r0 = o.forward(c["lat"], t, emb[:1], added(0))
        r1 = o.forward(c["lat"], t, emb[2:3], added(2), ctl={"fontsize": {"word_pos": c["wp"], "font_size": c["fs"]}})
        cap = {}
        r2 = o.forward(c["lat_ref"], t, emb[2:3], added(2), ctl={"capture": cap})
        inj = {k: v for k, v in cap.items() if k.endswith("attn1") or k == INJECT_RESNET}
        r3 = o.forward(c["lat"], t, emb[1:2], added(1), ctl={"inject": inj})
    return [r0[0], r1[0], r2[0], r3[0]]
