"""Test helper (not collected): the guided-prediction pre-pass (CFG rescale + v-prediction) and the five solvers' use of it, restated in
fp64 independently of csrc/guided.hip, csrc/step_driver.inl and the product's schedulers.py.

  * compose + CFG: tests/step_ref.py's rules (rd.py:119-132 / xl.py:810-825), with the conditional half kept beside the guided value.
  * the rescale factor: rescale_noise_cfg (xl.py:42-53): std over all 4 h w values, torch's unbiased default,
    f = phi std_text / std_cfg + (1 - phi); phi is the fp32 value the engine is handed.  The main stream uses (composed text, composed
    cfg); the reference pair its own (text_ref, cfg_ref) - the plain pass's treatment.
  * m = cfg f (phi > 0), then - v-prediction - eps = cv m + cx x with x the stream's own unscaled latent and (cv, cx) the level at which
    the UNet was evaluated: sigma space cv = 1 / sqrt(s_i^2 + 1), cx = s_i / (s_i^2 + 1); VP cv = sqrt(ac_t), cx = sqrt(1 - ac_t).
  * the solvers: PLMS and Euler are tests/step_ref.py's; DPM-Solver++ 2M, Euler ancestral and SDE-DPM-Solver++ 2M are restated here with
    magnitudes ([memory], the formulas of tests/dpm_solver_ref.py / tests/sde_ref.py, to which tests/test_guided_prediction.py pins them).

Every quantity is a (value, magnitude) pair as in step_ref.py: u * magnitude bounds what one fp32 rounding of any intermediate moves the
result.  Host scalars are pairs too (class Sc): a product multiplies magnitudes, log adds m / |v|, exp multiplies by (1 + m), so the
cancellation in exp(-h) - 1 or sigma_down - sigma is priced in.  The factor's magnitude is
    f + f (rms(mag_cfg) / std_cfg + rms(mag_text) / std_text):
its own rounding plus what one rounding of every composed value moves a standard deviation (|d std| <= rms(d x) by Cauchy-Schwarz).
"""
import math

import numpy as np
import torch

from tests import step_ref as S

KINDS = {"plms": 1, "euler": 0, "dpm2": 3, "euler_a": 4, "sde2": 6}          # the engine's schedule kinds
SIGMA_SPACE = ("euler", "euler_a")

MUTATIONS = (
    "biased_std",                 # n instead of n - 1 in BOTH standard deviations: cancels in the ratio (see test_guided_prediction.py)
    "biased_std_cfg",             # n instead of n - 1 in std_cfg only
    "std_base_text",              # std of the base stream's text prediction instead of the composed text
    "main_factor_on_pair",        # the main stream's factor applied to the reference pair
    "phi_swapped",                # (1 - phi) std_text / std_cfg + phi
    "cvcx_swapped",
    "cx_next_sigma",              # cx from the level the step lands on
    "pair_converted_with_lat",    # the pair's v -> eps conversion with the main latents
    "rescale_after_conversion",   # the factor applied to the eps-equivalent instead of the model output
)


# ---------------------------------------------------------------------------------------------------------- scalars with magnitudes
class Sc:
    def __init__(self, v, m=None):
        self.v, self.m = float(v), abs(float(v)) if m is None else float(m)

    @staticmethod
    def of(x):
        return x if isinstance(x, Sc) else Sc(x)

    def __add__(self, o):
        o = Sc.of(o); return Sc(self.v + o.v, self.m + o.m)

    def __sub__(self, o):
        o = Sc.of(o); return Sc(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return Sc.of(o) - self

    def __mul__(self, o):
        o = Sc.of(o); return Sc(self.v * o.v, self.m * o.m)

    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Sc.of(o); return Sc(self.v / o.v, self.m / abs(o.v) * (o.m / abs(o.v)))

    def __rtruediv__(self, o):
        return Sc.of(o) / self

    def sqrt(self):
        r = math.sqrt(self.v); return Sc(r, r * (self.m / abs(self.v)) if self.v else 0.0)

    def log(self):
        return Sc(math.log(self.v), abs(math.log(self.v)) + self.m / abs(self.v))

    def exp(self):
        r = math.exp(self.v); return Sc(r, r * (1.0 + self.m))


def tmul(c, q):
    c = Sc.of(c); return c.v * q[0], c.m * q[1]


def tadd(*qs):
    return sum(q[0] for q in qs), sum(q[1] for q in qs)


def tneg(q):
    return -q[0], q[1]


# ---------------------------------------------------------------------------------------------------------- the three other solvers
def dpm_timesteps(n, num_train=1000):
    ts = np.linspace(0, num_train - 1, n + 1).round()[::-1][:-1].astype(np.int64)
    out = []
    for t in ts.tolist():
        if t not in out:
            out.append(t)
    return out


class _VP:
    """alpha, sigma, lambda of a timestep as Sc, in fp64 from the fp32 alphas_cumprod entry."""

    def __init__(self):
        self.ac = S.alphas_cumprod().double()

    def alpha(self, t):
        return Sc(self.ac[t].item()).sqrt()

    def sigma(self, t):
        return (1.0 - Sc(self.ac[t].item())).sqrt()

    def lam(self, t):
        return self.alpha(t).log() - self.sigma(t).log()


class DPM2(_VP):
    """DPM-Solver++(2M), midpoint, lower-order final step below 15 steps; per-row x0 history; `sde`: SDE-DPM-Solver++(2M) with the
    field noise_fn(i) [1,4,h,w] (fp64), the same for every row."""
    kind, sde = 3, False

    def __init__(self, n, mutations=(), noise_fn=None):
        super().__init__()
        self.n_steps, self.mut, self.noise_fn = n, set(mutations), noise_fn
        self.timesteps = dpm_timesteps(n)
        self.m1, self.lower = None, 0

    def table(self):
        return S.alphas_cumprod().tolist()

    def step(self, i, eps, x):
        ts, n = self.timesteps, len(self.timesteps)
        s0, p = ts[i], (0 if i == n - 1 else ts[i + 1])
        rows = x.shape[0]
        x0 = tmul(1.0 / self.alpha(s0), tadd(S.exact(x), tneg(tmul(self.sigma(s0), eps))))
        h = self.lam(p) - self.lam(s0)
        first = self.lower < 1 or i == 0 or (i == n - 1 and n < 15)
        if self.sde:
            q = 1.0 - (-2.0 * h).exp()
            c1 = self.alpha(p) * q
            out = tadd(tmul(self.sigma(p) / self.sigma(s0) * (-1.0 * h).exp(), S.exact(x)), tmul(c1, x0))
            sign = 1.0
        else:
            c1 = self.alpha(p) * ((-1.0 * h).exp() - 1.0)
            out = tadd(tmul(self.sigma(p) / self.sigma(s0), S.exact(x)), tneg(tmul(c1, x0)))
            sign = -1.0
        if not first:
            r0 = (self.lam(s0) - self.lam(ts[i - 1])) / h
            d1 = tmul(1.0 / r0, tadd(x0, tneg(S.rows(self.m1, 0, rows))))
            corr = tmul(0.5 * c1, d1)
            out = tadd(out, corr if sign > 0 else tneg(corr))
        if self.sde:
            z = self.noise_fn(i).double().expand_as(x)
            out = tadd(out, tmul(self.sigma(p) * q.sqrt(), S.exact(z)))
        if self.m1 is None or self.m1[0].shape[0] <= rows:
            self.m1 = x0
        else:                                   # shrinking batch: the stopped rows keep their (unused) history
            self.m1 = S.cat(x0, S.rows(self.m1, rows, self.m1[0].shape[0]))
        self.lower = min(self.lower + 1, 2)
        return out


class SDE2(DPM2):
    kind, sde = 6, True


class EulerA:
    kind = 4

    def __init__(self, n, mutations=(), noise_fn=None):
        self.n_steps, self.mut, self.noise_fn = n, set(mutations), noise_fn
        ts, sig = S.euler_schedule(n)
        self.timesteps = [float(t) for t in ts]
        self.sigmas = [float(s) for s in sig]

    def table(self):
        return self.sigmas

    def step(self, i, eps, x):
        s, sp = Sc(self.sigmas[i]), Sc(self.sigmas[i + 1])
        up = (sp * sp * (s * s - sp * sp) / (s * s)).sqrt()
        down = (sp * sp - up * up).sqrt()
        z = self.noise_fn(i).double().expand_as(x)
        return tadd(S.exact(x), tmul(down - s, eps), tmul(up, S.exact(z)))


def make_sched(kind, n, mutations=(), noise_fn=None):
    if kind in ("plms", "euler"):
        return S.make_sched(kind, n, mutations)
    return {"dpm2": DPM2, "sde2": SDE2, "euler_a": EulerA}[kind](n, mutations, noise_fn)


def init_sigma(kind, sched):
    return (sched.sigmas[0] ** 2 + 1) ** 0.5 if kind in SIGMA_SPACE else 1.0


# ---------------------------------------------------------------------------------------------------------- the pre-pass
def v_scalars(kind, sched, i, mutations=()):
    """(cv, cx) as Sc: the level at which the UNet of step i was evaluated."""
    j = i + 1 if "cx_next_sigma" in mutations else i
    if kind in SIGMA_SPACE:
        s, sx = Sc(sched.sigmas[i]), Sc(sched.sigmas[j])
        cv, cx = 1.0 / (s * s + 1.0).sqrt(), sx / (sx * sx + 1.0)
    else:
        ac = S.alphas_cumprod().double()
        ts = sched.timesteps
        tj = int(ts[j]) if j < len(ts) else 0
        a, ax = Sc(ac[int(ts[i])].item()), Sc(ac[tj].item())
        cv, cx = a.sqrt(), (1.0 - ax).sqrt()
    return (cx, cv) if "cvcx_swapped" in mutations else (cv, cx)


def std_of(q, biased=False):
    x = q[0].reshape(-1).double()                # fp64 accumulation, as the kernel's
    n = x.numel()
    return math.sqrt(((x * x).sum().item() - x.sum().item() ** 2 / n) / (n if biased else n - 1))


def factor(text, cfg, phi, mutations=()):
    """f = phi std_text / std_cfg + (1 - phi) as Sc (phi already the fp32 value)."""
    mut = set(mutations)
    st = std_of(text, "biased_std" in mut)
    sc = std_of(cfg, "biased_std" in mut or "biased_std_cfg" in mut)
    a, b = (1.0 - phi, phi) if "phi_swapped" in mut else (phi, 1.0 - phi)
    f = a * st / sc + b
    rms = lambda q: math.sqrt((q[1] * q[1]).mean().item())
    return Sc(f, abs(f) * (1.0 + rms(cfg) / sc + rms(text) / st))


def phi32(phi):
    return float(np.float32(phi))


def guide(text, cfg, x, phi, vpred, cvcx, f=None, mutations=()):
    """(text, cfg) pairs [1,4,h,w], x exact -> (the eps-equivalent guided prediction, the factor)."""
    mut = set(mutations)
    if phi > 0 and f is None:
        f = factor(text, cfg, phi, mut)
    m = cfg
    late = "rescale_after_conversion" in mut and vpred
    if phi > 0 and not late:
        m = tmul(f, m)
    if vpred:
        m = tadd(tmul(cvcx[0], m), tmul(cvcx[1], S.exact(x)))
    if phi > 0 and late:
        m = tmul(f, m)
    return m, f


def compose(ep, M, g):
    """(composed text, guided value) of the main stream of a rich step."""
    R = len(M)
    nu = S.lin((M[-1], ep["u"]), *[(M[r], ep["u"]) for r in range(R - 1)])
    nt = S.lin((M[-1], ep["b"]), *[(M[r], ep[f"r{r}"]) for r in range(R - 1)])
    return nt, S.cfg(nu, nt, g)


def plain_step(kind, sched, i, eu, et, x, g, phi=0.0, vpred=False, mutations=()):
    """-> dict(lat, noise_pred (the eps-equivalent), factor)."""
    text, cfg = S.exact(et), S.cfg(S.exact(eu), S.exact(et), g)
    e, f = guide(text, cfg, x, phi, vpred, v_scalars(kind, sched, i, mutations) if vpred else None, mutations=mutations)
    return dict(lat=sched.step(i, e, x), noise_pred=e, factor=f)


def rich_step(kind, sched, i, ep, M, x, x_ref, g, isa, ibg, xl, elide=False, phi=0.0, vpred=False, mutations=()):
    mut = set(mutations)
    p = S.plan(i, sched.timesteps, len(M), isa, ibg, xl, elide)
    q = {k: S.exact(v) for k, v in ep.items()}
    text, cfg = compose(q, M, g)
    if "std_base_text" in mut:
        text = q["b"]
    cvcx = v_scalars(kind, sched, i, mut) if vpred else None
    e, f = guide(text, cfg, x, phi, vpred, cvcx, mutations=mut)
    f_ref = None
    if p["step_ref"]:
        text_r, cfg_r = q["tr"], S.cfg(q["ur"], q["tr"], g)
        er, f_ref = guide(text_r, cfg_r, x if "pair_converted_with_lat" in mut else x_ref, phi, vpred, cvcx,
                          f=f if "main_factor_on_pair" in mut else None, mutations=mut)
        out = sched.step(i, S.cat(e, er), torch.cat([x, x_ref]))
        lat, lat_ref = S.rows(out, 0, 1), S.rows(out, 1, 2)
    else:
        lat, lat_ref = sched.step(i, e, x), S.exact(x_ref)
    if p["blend"]:
        lat = S.lin((M[-1], lat_ref), (1 - M[-1], lat))
    return dict(lat=lat, lat_ref=lat_ref, noise_pred=e, factor=f, factor_ref=f_ref, **p)


# ---------------------------------------------------------------------------------------------------------- the test matrix
SETTINGS = {"eps_phi": (False, 0.7), "v": (True, 0.0), "v_phi": (True, 0.7)}


def _c(name, kind, mode, setting, n=8, lat=(16, 16), eng=(32, 32), R=0, isa=0.0, ibg=0.0, elide=False, defer=False):
    vpred, phi = SETTINGS[setting]
    xl = kind in SIGMA_SPACE
    return dict(name=name, kind=kind, mode=mode, R=R, n=n, lat=lat, eng=eng, isa=isa, ibg=ibg, elide=elide, defer=defer, xl=xl,
                g=5.0 if xl else 7.5, vpred=vpred, phi=phi)


def _cases():
    out = []
    for k, kind in enumerate(KINDS):
        for s, setting in enumerate(SETTINGS):
            # plain: one full block or one partial block; rich: 960 pixels = three full blocks and a 192-pixel tail, R = 4 with the pair
            small = dict(lat=(12, 8), eng=(32, 32)) if (k + s) % 2 else dict(lat=(16, 16), eng=(32, 32))
            out.append(_c(f"{kind}_plain_{setting}", kind, "plain", setting, n=6 + (k + s) % 5, **small))
            out.append(_c(f"{kind}_rich_{setting}", kind, "rich", setting, n=6 + (2 * k + s) % 5, lat=(24, 40), eng=(32, 48), R=4, isa=0.5,
                          ibg=0.3))
    # the pair stops part-way (t > 700 up to step 2, blend at int(0.2 * 10) = 2); a blend deferred behind the step
    out.append(_c("dpm2_elided_v_phi", "dpm2", "rich", "v_phi", n=10, lat=(12, 8), eng=(32, 32), R=4, isa=0.3, ibg=0.2, elide=True))
    out.append(_c("euler_deferred_v_phi", "euler", "rich", "v_phi", n=10, lat=(16, 16), eng=(32, 32), R=4, isa=0.5, ibg=0.3, defer=True))
    return out


CASES = _cases()
CASE = {c["name"]: c for c in CASES}


def case_inputs(case, seed=0):
    """Seeded fp32 inputs: x_T [1,4,h,w], R masks (a partition of unity), per step a model output for every role."""
    h, w = case["lat"]
    g = torch.Generator().manual_seed(2000 + 7 * seed + sum(map(ord, case["name"])))
    R = max(case["R"], 1)
    m = torch.softmax(torch.randn(R, 1, h, w, generator=g) * 2, 0).repeat(1, 4, 1, 1)
    sched = make_sched(case["kind"], case["n"])
    x = torch.randn(1, 4, h, w, generator=g) * init_sigma(case["kind"], sched)
    steps = [{k: torch.randn(1, 4, h, w, generator=g) for k in S.roles(R)} for _ in sched.timesteps]
    return x, [m[r:r + 1] for r in range(R)], steps


def step_once(case, sched, i, ep, M, lat, lat_ref, mutations=(), elide=None):
    """One step of the case from exact fp64 states -> rich_step's / plain_step's dict."""
    kw = dict(phi=phi32(case["phi"]), vpred=case["vpred"], mutations=mutations)
    if case["mode"] == "plain":
        return plain_step(case["kind"], sched, i, ep["u"], ep["b"], lat, case["g"], **kw)
    return rich_step(case["kind"], sched, i, ep, M, lat, lat_ref, case["g"], case["isa"], case["ibg"], case["xl"],
                     case["elide"] if elide is None else elide, **kw)


def one_step_margins(case, mutations, noise_fn=None):
    """Largest max|mutated - unmutated| / max(bar) over every one-step output (lat, lat_ref) of the case, both stepped from the
    unmutated trajectory; the solver histories of the two are kept apart."""
    x, M, steps = case_inputs(case)
    x, M = x.double(), [m.double() for m in M]
    good, bad = make_sched(case["kind"], case["n"], noise_fn=noise_fn), make_sched(case["kind"], case["n"], noise_fn=noise_fn)
    lat, lat_ref, worst = x, x.clone(), 0.0
    for i, ep in enumerate(steps):
        ep = {k: v.double() for k, v in ep.items()}
        a = step_once(case, good, i, ep, M, lat, lat_ref)
        b = step_once(case, bad, i, ep, M, lat, lat_ref, mutations)
        for k in ("lat", "lat_ref"):
            if k in a:
                worst = max(worst, (a[k][0] - b[k][0]).abs().max().item() / (S.ULPS * S.U32 * a[k][1].max().item()))
        lat = a["lat"][0]
        lat_ref = a["lat_ref"][0] if "lat_ref" in a else lat_ref
    return worst
