"""Test helper (not collected): the image start restated in fp64 for the tests, independently of the product's schedulers.py and
csrc/step.hip.  It plays the role dpm_solver_ref.py plays for DPM-Solver++.

  * ref_schedule(kind, n, strength): the truncated tables, start level and per-iteration source levels.  The FULL tables come from the
    oracle's schedulers (oracle/schedulers.py, tests/dpm_solver_ref.py); the truncation rule is restated here:
        k = min(int(n * strength), n) solver steps run, t_start = n - k
        euler: timesteps[t_start:], sigmas[t_start:]            dpm: timesteps[t_start:]
        pndm : the distinct descending timesteps D, D[t_start:] expanded as [d0, d1, d1, d2, ...] (k + 1 iterations)
  * euler_loop / plms_loop / dpm_loop: the three solvers in fp64, driven by those tables and a noise-prediction callback
  * noise_latents_ref / source_blend_ref / blend_bound: the two kernels of csrc/step.hip in fp64 and the fp32 error bound of the tests
"""
import numpy as np
import torch

from oracle.schedulers import OracleEuler, OraclePNDM, scaled_linear_alphas_cumprod
from tests.dpm_solver_ref import dpm_timesteps


def executed_steps(n, strength, least=1):
    if not (0.0 < strength <= 1.0):
        raise ValueError("strength")
    k = min(int(n * strength), n)
    if k < least:
        raise ValueError("too few steps")
    return k


def vp_level(ac64, t):
    a = float(ac64[int(t)])
    return a ** 0.5, (1.0 - a) ** 0.5


def ref_schedule(kind, n, strength=1.0):
    """kind 'euler' | 'pndm' | 'dpm' -> dict(timesteps, sigmas (euler), ac (fp64 table), start=(a, b), levels=[(a, b)] per iteration)."""
    ac = scaled_linear_alphas_cumprod().double().numpy()
    if kind == "euler":
        k = executed_steps(n, strength)
        o = OracleEuler(); o.set_timesteps(n)
        ts, sig = o.timesteps.numpy()[n - k:], o.sigmas.numpy()[n - k:]
        return dict(timesteps=ts, sigmas=sig, ac=ac, start=(1.0, float(sig[0])),
                    levels=[(1.0, float(s)) for s in sig[1:-1]] + [(1.0, 0.0)])
    if kind == "pndm":
        k = executed_steps(n, strength, least=2)
        o = OraclePNDM(); o.set_timesteps(n)
        D = sorted(set(o.timesteps.tolist()), reverse=True)
        assert len(D) == n
        d = D[n - k:]
        ts = np.array([d[0], d[1]] + d[1:], dtype=np.int64)
        lands = [d[1], d[1]] + d[2:]
        return dict(timesteps=ts, ac=ac, start=vp_level(ac, d[0]), levels=[vp_level(ac, t) for t in lands] + [(1.0, 0.0)])
    if kind == "dpm":
        k = executed_steps(n, strength)
        ts = dpm_timesteps(n)[n - k:]
        if len(ts) == 0:
            raise ValueError("too few steps")
        return dict(timesteps=ts, ac=ac, start=vp_level(ac, ts[0]), levels=[vp_level(ac, t) for t in ts[1:]] + [(1.0, 0.0)])
    raise KeyError(kind)


# ---- the solvers in fp64.  eps_fn(x, i, t) -> noise prediction at iteration i; returns (final x, [x after every iteration])
def euler_loop(timesteps, sigmas, x, eps_fn):
    s = np.asarray(sigmas, dtype=np.float64)
    x, trace = x.double().clone(), []
    for i, t in enumerate(timesteps):
        x = x + eps_fn(x, i, float(t)) * (s[i + 1] - s[i])
        trace.append(x.clone())
    return x, trace


def plms_loop(timesteps, ac, n_full, x, eps_fn, num_train=1000):
    """PNDMScheduler.step_plms (skip_prk_steps, steps_offset 1, set_alpha_to_one False); the step ratio is the FULL schedule's."""
    ratio = num_train // n_full
    ets, counter, cur = [], 0, None
    x, trace = x.double().clone(), []

    def prev(sample, t, p, e):
        a_t, a_p = ac[t], (ac[p] if p >= 0 else ac[0])
        b_t, b_p = 1 - a_t, 1 - a_p
        return (a_p / a_t) ** 0.5 * sample - (a_p - a_t) * e / (a_t * b_p ** 0.5 + (a_t * b_t * a_p) ** 0.5)

    for i, t in enumerate(int(v) for v in timesteps):
        e = eps_fn(x, i, t)
        p = t - ratio
        sample = x
        if counter != 1:
            ets = ets[-3:] + [e]
        else:
            p, t = t, t + ratio
        if len(ets) == 1 and counter == 0:
            cur = sample
        elif len(ets) == 1 and counter == 1:
            e, sample = (e + ets[-1]) / 2, cur
        elif len(ets) == 2:
            e = (3 * ets[-1] - ets[-2]) / 2
        elif len(ets) == 3:
            e = (23 * ets[-1] - 16 * ets[-2] + 5 * ets[-3]) / 12
        else:
            e = (55 * ets[-1] - 59 * ets[-2] + 37 * ets[-3] - 9 * ets[-4]) / 24
        x = prev(sample, t, p, e)
        counter += 1
        trace.append(x.clone())
    return x, trace


def dpm_loop(timesteps, ac, order, x, eps_fn):
    """DPM-Solver++ multistep (midpoint, epsilon, lower_order_final counted on the list that is executed)."""
    ac = np.asarray(ac, dtype=np.float64)
    alpha, sigma = np.sqrt(ac), np.sqrt(1 - ac)
    lam = np.log(alpha) - np.log(sigma)
    ts = [int(t) for t in timesteps]
    n = len(ts)
    x, trace, m1, lower = x.double().clone(), [], None, 0
    for i, s0 in enumerate(ts):
        p = 0 if i == n - 1 else ts[i + 1]
        x0 = (x - sigma[s0] * eps_fn(x, i, s0)) / alpha[s0]
        h = lam[p] - lam[s0]
        c1 = alpha[p] * (np.exp(-h) - 1.0)
        new = (sigma[p] / sigma[s0]) * x - c1 * x0
        if not (order == 1 or lower < 1 or (i == n - 1 and n < 15)):
            r0 = (lam[s0] - lam[ts[i - 1]]) / h
            new = new - 0.5 * c1 * (1.0 / r0) * (x0 - m1)
        x, m1, lower = new, x0, min(lower + 1, order)
        trace.append(x.clone())
    return x, trace


# ---- the two kernels.  a, b are what the kernels receive: the levels rounded to fp32 at the C boundary.
def _f32(v):
    return float(np.float32(v))


def noise_latents_ref(x0, noise, a, b):
    return _f32(a) * x0.double() + _f32(b) * noise.double()


def source_blend_ref(lat, x0, noise, keep, a, b):
    """keep [h,w] broadcast over the four channels of lat / x0 / noise [1,4,h,w]."""
    k = keep.double().reshape(1, 1, *keep.shape[-2:])
    return k * noise_latents_ref(x0, noise, a, b) + (1.0 - k) * lat.double()


def blend_bound(lat, x0, noise, a, b):
    """|err| <= 4 * 2^-24 * (|a x0| + |b noise| + |lat|) per element: the expression has at most four fp32 roundings on the path of any
    one of its terms."""
    return 4.0 * 2.0 ** -24 * ((_f32(a) * x0.double()).abs() + (_f32(b) * noise.double()).abs() + lat.double().abs())
