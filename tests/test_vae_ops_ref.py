"""The references of the VAE's per-kernel GPU tests (tests/vae_ops_ref.py) on the CPU, for exactly the inputs tests/test_vae_ops_gpu.py
uses: each reference against an independent statement of the operator, the distance of an honest fp32 evaluation from it (the
"noise": what no bar may be confused by), and every emulated fault against its bar.

Per kernel and input set, with `bar` the constant the GPU test asserts (8 x the error measured on the MI355X) and `ceiling` the
smallest emulated fault / 10, the largest value a bar may ever take (faults are measured beyond the plane rounding 2^-8 |ref| the GPU
test allows on bf16 outputs):
    every fault >= 10 x bar      the test bites
    bar <= ceiling               (the same statement; for the contraction the ceiling is the 4e-4 of the issue)
    100 x noise <= ceiling       the fp32 control sits two decades under anything a bar here may become
    noise <= bar                 ... and under the bar itself: an honest fp32 kernel passes
The measured bars are 8 x the kernels' own fp32 error, i.e. one decade above the noise, not two; the factor 100 is therefore proven
against the ceiling.  Inputs are chosen so that all of this holds (dA = randn + 0.75 + 0.75 xh; dP with a per-row constant; colour
images on a dyadic grid)."""
import pytest
import torch

import vae_ops_ref as R
from memcases import HILO_CASES, hilo_id


def margins(name, bar, noise, faults, ceiling=None):
    """faults: {label: metric}."""
    worst = min(faults.values())
    ceiling = worst / 10 if ceiling is None else ceiling
    print(f"{name}: bar {bar:.3e} noise {noise:.3e} ceiling {ceiling:.3e} faults " + " ".join(f"{k}={v:.3e}" for k, v in faults.items()))
    assert all(v >= 10 * bar for v in faults.values()), (name, bar, faults)
    assert bar <= ceiling and ceiling <= worst / 10
    assert 100 * noise <= ceiling, (name, noise, ceiling)
    assert noise <= bar, (name, noise, bar)


# ----------------------------------------------------------------------------------------------------------------- contraction
def _shape_key(c):
    return tuple(c[k] for k in ("mode", "bias", "wact") if k in c) + (bool(c["res"]),) + R.hilo_shape(c)


HILO_UNIQUE = list({_shape_key(c): c for c in HILO_CASES}.values())


@pytest.mark.parametrize("case", HILO_UNIQUE, ids=hilo_id)
def test_contraction_reference_noise_and_faults(case):
    A, W, bias, res = R.hilo_inputs(case)
    ref = R.t3(case, A, W, bias, res)
    M, N, K, Ho, Wo = R.hilo_shape(case)
    assert ref.dtype == torch.float64 and ref.shape == (M, N)
    if case["mode"] != 0:
        # the im2col statement of the convolution against torch's own convolution of the same planes (stride / padding / up-sample by torch)
        x = A[0].double().permute(2, 0, 1)[None]
        w4 = W[0].double().reshape(N, 3, 3, case["Cin"]).permute(0, 3, 1, 2)
        if case["mode"] == 3:
            x = torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")
        y = torch.nn.functional.conv2d(torch.nn.functional.pad(x, (0, 1, 0, 1)), w4, stride=2) if case["mode"] == 4 else torch.nn.functional.conv2d(x, w4, padding=1)
        mine = R.im2col(A[0].double(), case["mode"], Ho, Wo) @ W[0].double().t()
        assert (y[0].permute(1, 2, 0).reshape(M, N) - mine).abs().max().item() < 1e-11
    # T3 is the product of the pairs up to the dropped lo.lo term (2^-18 relative per product)
    full = R.t3(case, (R.pair64(*A), torch.zeros_like(A[0])), (R.pair64(*W), torch.zeros_like(W[0])), bias, res)
    assert R.max_over_rms(ref, full) < 2.0 ** -15
    noise = R.max_over_rms(R.t3(case, A, W, bias, res, dtype=torch.float32), ref)
    faults = {f: R.max_over_rms(R.t3(case, A, W, bias, res, fault=f), ref) for f in R.HILO_FAULTS if R.hilo_fault_applies(case, f)}
    margins(hilo_id(case), R.bar("contraction"), noise, faults, ceiling=R.CONTRACTION_CEILING)
    # the single-pass call differs from T3 by the two lo passes: the F32_OUT bar of the existing tests (2e-3 + 2e-3 |ref|) holds for it
    one = R.t3(case, A, W, bias, res, single=True)
    assert 1e-3 < R.max_over_rms(one, ref) < 2e-2


def test_split_values_cover_the_edges():
    for n in R.SPLIT_SIZES:
        x = R.split_values(n)
        hi, lo = R.split(x)
        assert n % 4 == 0 and x.shape == (n,)
        v = hi.double() + lo.double()
        nz = x != 0
        assert ((v - x.double()).abs()[nz] / x.double().abs()[nz]).max().item() <= 2.0 ** -16
    x = R.split_values(R.SPLIT_SIZES[0])
    hi, lo = R.split(x)
    assert hi[0].item() == 0 and hi[1].item() == 0 and torch.signbit(hi[1]) and not torch.signbit(hi[0])
    exact = (hi.double() + lo.double()) == x.double()
    assert bool(exact[6:10].all()) and lo[6].item() == 2.0 ** -9 and hi[6].item() == 1.0
    assert torch.isfinite(hi.float()).all() and torch.isfinite(lo.float()).all() and lo[2].item() != 0


# ----------------------------------------------------------------------------------------------------------------- GroupNorm
GN_RUNS = list(zip(R.GN_CASES, R.GN_VARIANTS))


@pytest.mark.parametrize("case,v", GN_RUNS, ids=[R.gn_id(c, v) for c, v in GN_RUNS])
def test_groupnorm_references_noise_and_faults(case, v):
    Cc, G, HW, B = case
    x, gamma, beta, dA, add = R.gn_inputs(case, v)
    da = R.pair64(*dA)
    ref = R.gn_bwd_ref(x, da, G, gamma, beta, v["silu"], add)
    mean, rstd = R.gn_stats(x.double(), G)
    # autograd through the whole operator == the closed formula of csrc/common.h with the exact statistics
    closed = R.gn_bwd_formula(x, da, mean, rstd, G, gamma, beta, v["silu"], add)
    assert R.needed_R(closed, ref) < 1e-11
    # forward reference against torch's group_norm
    y, m2, r2 = R.gn_fwd_ref(x, G, gamma, beta, v["silu"])
    t = torch.nn.functional.group_norm(x.double().transpose(1, 2), G, gamma.double(), beta.double(), R.GN_EPS).transpose(1, 2)
    assert R.needed_R(y, torch.nn.functional.silu(t) if v["silu"] else t) < 1e-12
    # noise: the formula in fp32 from fp32-rounded statistics
    noise = R.needed_R(R.gn_bwd_formula(x, da, mean.float(), rstd.float(), G, gamma, beta, v["silu"], add, dtype=torch.float32), ref)
    # what the GPU test allows on top of the bar: the rounding of the planes where no fp32 output is asked for
    rel = 0.0 if v["out"] else (R.PAIR_REL if v["out_lo"] else R.HI_REL)
    faults = {f: R.needed_R(R.gn_bwd_formula(x, da, mean, rstd, G, gamma, beta, v["silu"], add, fault=f), ref, rel=rel)
              for f in R.GN_BWD_FAULTS if v["silu"] or f != "sigmoid_only"}
    faults["rel_l2(drop_mean_dxh)"] = R.rel_l2(R.gn_bwd_formula(x, da, mean, rstd, G, gamma, beta, v["silu"], None, fault="drop_mean_dxh"),
                                               R.gn_bwd_formula(x, da, mean, rstd, G, gamma, beta, v["silu"], None))
    assert faults.pop("rel_l2(drop_mean_dxh)") > 0.3                 # the issue's 72..85 % class, not the 2.6 % of an uncorrelated dA
    for name in ("gn_bwd", "gn_bwd_exact"):
        margins(R.gn_id(case, v) + " " + name, R.bar(name), noise, faults)
    fnoise = R.needed_R(R._silu_or_id((x - R._per_channel(mean.float(), Cc)) * R._per_channel(rstd.float(), Cc) * gamma + beta, v["silu"]), y)
    wrong = R._silu_or_id((x.double() - R._per_channel(mean.roll(1, 1), Cc)) * R._per_channel(rstd.roll(1, 1), Cc) * gamma.double() + beta.double(), v["silu"])
    no_beta = R._silu_or_id((x.double() - R._per_channel(mean, Cc)) * R._per_channel(rstd, Cc) * gamma.double(), v["silu"])
    margins(R.gn_id(case, v) + " gn_fwd", R.bar("gn_fwd"), fnoise, {"wrong_group_stats": R.needed_R(wrong, y, rel=R.HI_REL), "no_beta": R.needed_R(no_beta, y, rel=R.HI_REL)})


# ----------------------------------------------------------------------------------------------------------------- softmax
@pytest.mark.parametrize("rows,cols", R.SOFTMAX_CASES)
def test_softmax_references_noise_and_faults(rows, cols):
    s = R.softmax_scores(rows, cols)
    ref = R.softmax_ref(s)
    assert (ref.sum(-1) - 1).abs().max().item() < 1e-14 and ref[rows - 1].max().item() > 0.999
    noise = R.needed_R(torch.softmax(s * R.SOFTMAX_SCALE, dim=-1), ref)
    e = (s.double() * R.SOFTMAX_SCALE - (s.double() * R.SOFTMAX_SCALE).amax(-1, keepdim=True)).exp()
    faults = {"no_scale": R.needed_R(torch.softmax(s.double(), -1), ref, rel=R.HI_REL),
              "last_column_not_summed": R.needed_R(e / e[:, :-1].sum(-1, keepdim=True), ref, rel=R.HI_REL)}
    margins(f"softmax {rows}x{cols}", R.bar("softmax"), noise, faults)
    for with_lo in (True, False):
        P, dp = R.softmax_bwd_inputs(rows, cols, with_lo)
        bref = R.softmax_bwd_ref(P, dp)
        # the formula is the adjoint of softmax(scale s): autograd at unrounded probabilities
        s0 = torch.randn(rows, cols, dtype=torch.float64, generator=R.gen(3)).requires_grad_(True)
        p0 = torch.softmax(s0 * R.SOFTMAX_SCALE, -1)
        (p0 * dp.double()).sum().backward()
        assert R.needed_R(R.softmax_bwd_ref((p0.detach(), None), dp), s0.grad) < 1e-12
        bnoise = R.needed_R(R.softmax_bwd_ref(P, dp, dtype=torch.float32), bref)
        rel = R.PAIR_REL if with_lo else R.HI_REL                     # the plane rounding the GPU test allows for this output
        bf = {f: R.needed_R(R.softmax_bwd_ref(P, dp, fault=f), bref, rel=rel) for f in R.SOFTMAX_BWD_FAULTS + (("dot_of_hi_only",) if with_lo else ())}
        margins(f"softmax_bwd {rows}x{cols} lo={with_lo}", R.bar("softmax_bwd"), bnoise, bf)


# ----------------------------------------------------------------------------------------------------------------- sum-pool, pq_conv
def test_sumpool_and_pq_conv_references():
    for B, H, W, Cc in R.SUMPOOL_CASES[:2]:
        x = torch.randn(B, 2 * H, 2 * W, Cc, generator=R.gen(61))
        ref, terms = R.sumpool_ref(x)
        want = 4 * torch.nn.functional.avg_pool2d(x.double().permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1)
        assert (ref - want).abs().max().item() < 1e-13
        f32 = x.reshape(B, H, 2, W, 2, Cc).sum(dim=(2, 4))
        assert bool(((f32.double() - ref).abs() <= 2.0 ** -22 * terms).all())                  # three fp32 additions: 3 x 2^-24 of the partial sums
        shifted = R.sumpool_ref(torch.roll(x, 1, dims=2))[0]
        assert ((shifted - ref).abs() > 2.0 ** -22 * terms * 10).float().mean().item() > 0.99
    for HW in R.PQ_HW:
        lat, eps, W, b, c_lat, c_eps = R.pq_inputs(HW)
        for e in (eps, None):
            ref, terms = R.pq_fwd_ref(lat, e, c_lat, c_eps, W, b)
            f32, _ = R.pq_fwd_ref(lat, e, c_lat, c_eps, W, b, dtype=torch.float32)
            assert bool(((f32.double() - ref).abs() <= 2.0 ** -21 * terms).all())
            hi, lo = R.split(f32)
            assert bool(((R.pair64(hi, lo) - ref).abs() <= R.PAIR_REL * ref.abs() + 2.0 ** -21 * terms).all())
            assert bool(((hi.double() - ref).abs() <= R.HI_REL * ref.abs() + 2.0 ** -21 * terms).all())
            wrong = R.pq_fwd_ref(lat, e, c_lat, c_eps, W.t(), b)[0]
            assert ((wrong - ref).abs() > 10 * (R.HI_REL * ref.abs() + 2.0 ** -21 * terms)).float().mean().item() > 0.9
        g = R.gen(71 + HW)
        dz, mask = torch.randn(HW, 4, generator=g), torch.rand(4, HW, generator=g)
        gr, new, tg, tn = R.pq_bwd_ref(dz, W, c_lat, 0.7, mask, lat)
        g32, n32, _, _ = R.pq_bwd_ref(dz, W, c_lat, 0.7, mask, lat, dtype=torch.float32)
        assert bool(((g32.double() - gr).abs() <= 2.0 ** -21 * tg).all()) and bool(((n32.double() - new).abs() <= 2.0 ** -21 * tn).all())
        gw, nw, _, _ = R.pq_bwd_ref(dz, W, c_lat, 0.7, mask, lat, fault="w_not_transposed")
        assert ((gw - gr).abs() > 10 * 2.0 ** -21 * tg).float().mean().item() > 0.95 and ((nw - new).abs() > 10 * 2.0 ** -21 * tn).float().mean().item() > 0.9
        # the update is autograd's: d/dlat of <dz, W (c lat) + b>
        l = lat.double().clone().requires_grad_(True)
        (R.pq_fwd_ref(l, None, c_lat, 0.0, W, b)[0] * dz.double()).sum().backward()
        assert (l.grad - gr).abs().max().item() < 1e-12


# ----------------------------------------------------------------------------------------------------------------- colour loss
@pytest.mark.parametrize("n", R.COLOR_N)
def test_color_reference_noise_and_faults(n):
    img, masks, target = R.color_inputs(n)
    loss, grad = R.color_ref(img, masks, target)
    # the grid: v and the clamp decision are exact in fp32; +-1 and both neighbours are present in every channel
    v32, v64 = img * 0.5 + 0.5, img.double() * 0.5 + 0.5
    assert torch.equal(v32.double(), v64) and bool((img * 1024 == (img * 1024).round()).all()) and img.abs().max().item() == 1.5
    for ch in range(3):
        col = set((img[:, ch] * 1024).int().tolist())
        assert {1024, -1024, 1025, -1025, 1023, -1023} <= col
    # against autograd through torch.clamp
    x = img.double().clone().requires_grad_(True)
    c = (x * 0.5 + 0.5).clamp(0.0, 1.0)
    avg = (masks.double() @ c) / masks.double().sum(-1, keepdim=True)
    L = (100.0 * (avg - target.double()).pow(2).mean(-1)).sum()
    L.backward()
    assert abs(L.item() - loss.item()) <= 1e-12 * abs(loss.item()) and R.needed_R(x.grad, grad) < 1e-12
    assert bool((grad[(v64 < 0).any(-1) & (v64 < 0).all(-1)] == 0).all())
    l32, g32 = R.color_ref(img, masks, target, dtype=torch.float32)
    gnoise, lnoise = R.needed_R(g32, grad), abs(l32.item() - loss.item()) / abs(loss.item())
    gf, lf = {}, {}
    for f in R.COLOR_FAULTS:
        lw, gw = R.color_ref(img, masks, target, fault=f)
        gf[f] = R.needed_R(gw, grad, rel=R.HI_REL)
        if f == "no_clamp_in_sums":
            lf[f] = abs(lw.item() - loss.item()) / abs(loss.item())
    margins(f"color_grad n={n}", R.bar("color_grad"), gnoise, gf)
    margins(f"color_loss n={n}", R.bar("color_loss"), lnoise, lf)
