"""References for perturbed-attention guidance (csrc/pag.hip, include/rtdiff.h: rt_set_pag_layers / rt_set_pag_scales).  Test
infrastructure, plain torch.

  PagOracleUNet         oracle.unet.OracleUNet whose applied attn1 modules return to_out.0(to_v(x)): no Q, no K, no softmax.  With an empty
                        applied set it is OracleUNet.
  all_attn1(cfg)        the attn1 module names of a config, in execution order (from the engine's own module table: no device needed)
  guidance_ref          the fp64 restatement the tests pin: eps = u + g (sum_r m_r T_r - u) + sum_r m_r sigma_r (T_r - P_r)
  fold_ref / fold_bar   the fold of a step in fp64 and its per-element bar
  rich_step_pag         the forwards of one rich step with twins on the oracle and the folded guidance: (eps, eps_ref)
"""
import torch

from oracle.region_loop import _fontsize
from oracle.unet import INJECT_RESNET, OracleUNet


# Guidance scale of the step tests on controlnet_ref.rich_case(): with sigma = (base 3.0, region 0 2.0, region 1 0) the oracle's latent
# update with PAG is 0.292 / 0.447 (main / reference stream) from the one without at the case's own g = 5, a hair under the 10 x STEP_BAR
# tests/test_pag.py asks for; at g = 3 the PAG term weighs 5 / 3 as much.  Chosen on the CPU oracle alone.
# What the engine can reach at STEP_BAR: every stream of a forward is eps = 8e-3 of its oracle in relative L2 (tests/test_pag_gpu.py, the
# forward test), and the guided prediction is (1 - g) u + (g + sigma) T - sigma P.  With independent stream errors of eps |T| the error
# of the prediction is eps |T| sqrt((g - 1)^2 + (g + sigma)^2 + sigma^2): 9.4 eps |T| at g = 5, sigma = 3 against 6.4 eps |T| without PAG
# (sigma = 0), and 7.0 eps |T| at g = 3.  The step bar was set for the two-term guidance at g = 5 (6.4 eps |T|; this case measures 2.2e-2
# there without PAG); a third term raises the error by the factor 9.4 / 6.4 at the same g, which is the 3.2e-2 / 3.5e-2 measured, and
# g = 3 brings the same three-term composition back to 7.0 / 6.4 of what the bar was set for.  The margin is thin (2.4e-2 / 2.9e-2).
STEP_GS = 3.0


class PagOracleUNet(OracleUNet):
    """OracleUNet with perturbed self-attention at the modules of `applied` (full attn1 names)."""

    def __init__(self, config, state_dict, applied=()):
        super().__init__(config, state_dict)
        self.applied = frozenset(applied)

    def _attention(self, name, x, heads, ctx=None, fontsize=None, real_probs=None, capture=None):
        if name in self.applied and ctx is None:
            return self._lin(self._lin(x, name + ".to_v", bias=False), name + ".to_out.0"), None
        return super()._attention(name, x, heads, ctx=ctx, fontsize=fontsize, real_probs=real_probs, capture=capture)


def all_attn1(cfg):
    from rich_text_to_image_amd.engine import Engine
    from rich_text_to_image_amd.pag import attn1_names
    e = Engine(cfg, 8, 8, device=-1)
    try:
        return attn1_names(e.attn_modules())
    finally:
        e.close()


def guidance_ref(u, T, P, masks, sigmas, g):
    """u [.., 4, h, w]; T, P, masks: lists over the slots (P[r] None where sigma_r == 0); fp64."""
    u = u.double()
    text = sum(m.double() * t.double() for m, t in zip(masks, T))
    out = u + g * (text - u)
    for m, t, p, s in zip(masks, T, P, sigmas):
        if s != 0.0:
            out = out + m.double() * s * (t.double() - p.double())
    return out


def fold_ref(t, p, rho):
    """fp64 of eps[s] + rho (eps[s] - eps[twin])."""
    return t.double() + float(rho) * (t.double() - p.double())


def fold_bar(t, p, rho):
    """2^-23 (|rho| |t - p| + |ref|): the subtraction's rounding (half an ulp of t - p, times |rho|) and the fma's (half an ulp of the
    result), with a factor 2 of margin."""
    return 2.0 ** -23 * (abs(float(rho)) * (t.double() - p.double()).abs() + fold_ref(t, p, rho).abs())


def twin_forward(o_pag, x, t, emb, added, ctl=None):
    with torch.no_grad():
        return o_pag.forward(x, t, emb, added, ctl=ctl)


def rich_step_pag(o, o_pag, lat_in, lat_ref_in, t, embeds, added_fn, masks, tfd, feat, sigmas, g, step_ref=True):
    """One rich step's forwards on the plain oracle `o` and the twins on `o_pag`, composed with the three-term guidance.  embeds
    [negative, regions ..., base]; sigmas: the slot vector [negative (0), regions ..., base].  The reference pair runs (use_ref).
    Returns (eps of the main stream, eps of the reference pair), fp64."""
    R = len(masks)
    fs = {"fontsize": _fontsize(tfd)}
    with torch.no_grad():
        u = o.forward(lat_in, t, embeds[:1], added_fn(0))
        b = o.forward(lat_in, t, embeds[-1:], added_fn(-1), ctl=fs)
        ur = o.forward(lat_ref_in, t, embeds[:1], added_fn(0))
        cap = {}
        tr = o.forward(lat_ref_in, t, embeds[-1:], added_fn(-1), ctl={"capture": cap if feat else None})
        inj = {k: v for k, v in cap.items() if k.endswith("attn1") or k == INJECT_RESNET} if feat else None
        T, P = [], []
        for r in range(R - 1):
            T.append(o.forward(lat_in, t, embeds[r + 1:r + 2], added_fn(r + 1), ctl={"inject": inj}))
            # the twin of an injected region stream: injected probabilities at the modules that are not applied, text_ref's ResNet feature
            P.append(o_pag.forward(lat_in, t, embeds[r + 1:r + 2], added_fn(r + 1), ctl={"inject": inj}) if sigmas[r + 1] != 0.0 else None)
        T.append(b)
        P.append(o_pag.forward(lat_in, t, embeds[-1:], added_fn(-1), ctl=fs) if sigmas[R] != 0.0 else None)
        eps = guidance_ref(u, T, P, masks, [sigmas[r + 1] for r in range(R - 1)] + [sigmas[R]], g)
        eps_ref = ur.double() + g * (tr.double() - ur.double())
        if step_ref and sigmas[R] != 0.0:
            pr = o_pag.forward(lat_ref_in, t, embeds[-1:], added_fn(-1))
            eps_ref = eps_ref + sigmas[R] * (tr.double() - pr.double())
    return eps, eps_ref
