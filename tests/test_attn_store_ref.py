"""The fp64 reference of the token-map store kernels (tests/attn_store_ref.py) against the oracle's attention probabilities, and the
distance of its fp32 control - the term R_control of the GPU matrix's bar - on every shape and input family of that matrix."""
import pytest
import torch

from oracle.unet import attention_probs

import attn_store_ref as R


SHAPES = sorted({c[:6] for c in R.STORE_CASES} | {(H, N, N, (N + 31) // 32 * 32, N, d) for H, N, d in R.HANDOVER_SELF}
                | {(H, N, 77, 96, 96, 64) for H, N in R.HANDOVER_CROSS})


@pytest.mark.parametrize("H,N,NK,d", [(3, 272, 352, 80), (2, 64, 77, 160), (20, 128, 77, 64), (2, 80, 1312, 64), (5, 328, 328, 40)])
def test_reference_matches_the_oracles_attention_probs(H, N, NK, d):
    """probs_avg_ref reads the packed bf16 operands in the log2 domain; oracle.unet.attention_probs (get_attention_scores,
    attention_processor.py:359-407) reads per-head fp32 q, k and the scale d^-1/2.  Same operands, both ways."""
    DP = R.dp_of(d)
    q, k = R.make_qk(H, N, NK, NK + 19, d, "plain", R.case_seed(H, N, NK, d))
    Q, K = R.pack_heads(q, H, d, DP, R.q_scale(d)), R.pack_heads(k, H, d, DP)
    ref = R.probs_avg_ref(Q, K, H, d, DP, NK)
    assert ref.dtype == torch.float64 and ref.shape == (N, NK)
    assert (ref.sum(-1) - 1).abs().max().item() < 1e-12
    qh = (Q.float() / R.q_scale(d)).reshape(N, H, DP).permute(1, 0, 2)
    kh = K.float()[:NK].reshape(NK, H, DP).permute(1, 0, 2)
    orc = attention_probs(qh, kh, d ** -0.5).mean(0)
    err = (orc.double() - ref).abs().max().item()
    print(f"H={H} N={N} NK={NK} d={d}: max |oracle fp32 - ref fp64| = {err:.3e}")
    assert err < 1e-5
    # the two wrong references of the discrimination control are wrong
    assert (R.probs_avg_ref(Q, K, H, d, DP, NK, head0=True) - ref).abs().max().item() > 1e-4
    drop = R.probs_avg_ref(Q, K, H, d, DP, NK, drop_last=True)
    assert drop[:, NK - 1].abs().max().item() == 0.0 and (drop.sum(-1) - 1).abs().max().item() < 1e-12


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("H,N,NK,NKpad,NKrows,d", SHAPES)
def test_fp32_control_distance_from_the_reference(H, N, NK, NKpad, NKrows, d, family):
    """R_control of the bar: what the fp32 CPU control needs at A = 1e-7, and its rel-L2.  Bounded by what the fp32 format allows
    (attn_store_ref.control_bound); the bar itself must stay under the 1e-3 ceiling on every case."""
    DP = R.dp_of(d)
    q, k = R.make_qk(H, N, NK, NKrows, d, family, R.case_seed(H, N, NK, d, R.FAMILIES.index(family)))
    Q, K = R.pack_heads(q, H, d, DP, R.q_scale(d)), R.pack_heads(k, H, d, DP)
    ref = R.probs_avg_ref(Q, K, H, d, DP, NK)
    ctl = R.probs_avg_fp32(Q, K, H, d, DP, NK)
    Rc, l2, smax = R.needed_R(ctl, ref, R.A_CONTROL), R.rel_l2(ctl, ref), R.max_abs_score(Q, K, H, DP, NK)
    bound = R.control_bound(smax, NK)
    print(f"control {family} H={H} N={N} NK={NK} d={d}: R_control={Rc:.3e} (bound {bound:.3e}) rel-L2={l2:.3e} |s|max={smax:.1f} bar R={R.bar_R(Rc, NKpad):.3e}")
    assert torch.isfinite(ctl).all() and (ref > 0).all()
    assert Rc <= bound and l2 <= bound
    assert R.bar_R(Rc, NKpad) <= 1e-3
    if family == "spiked":
        assert smax > 0.98 * 1600.0 * R.q_scale(d)               # the offset family really sits far from zero: 40 * 40 * d^-1/2 log2 e (bf16)
