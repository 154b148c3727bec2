"""Test helper (not collected): the PLMS / Euler step epilogue of the rich-text loops restated in fp64, written independently of
csrc/step.hip, csrc/step_driver.inl, the product's schedulers.py and oracle/.

  * PLMS: PNDMScheduler.step_plms (diffusers 0.18.2, [memory]) with skip_prk_steps, steps_offset 1, set_alpha_to_one=False.
  * Euler: EulerDiscreteScheduler (SDXL config, leading spacing, steps_offset 1), epsilon prediction, gamma = 0.
  * The rich-text step rules of models/region_diffusion.py:99-173 / models/region_diffusion_sdxl.py:779-872: region combine, CFG, when
    the reference pair is stepped, the blend index; plus the engine's elision rule (the reference pair stops once nothing reads it).
  * The plain step (rd.py:200-214 / xl.py:880-905).

Every quantity is carried as a pair (value, magnitude): the magnitude is the same expression evaluated on absolute values, so that
u * magnitude (u = 2^-24) bounds what one fp32 rounding of any intermediate can move the result.  The GPU tests compare at a few u of it.

`mutations` switches on named, deliberately wrong variants (MUTATIONS); tests/test_step_ref.py shows that each of them moves a one-step
output far beyond the GPU bar, which is the evidence that the bar catches subtle bugs.
"""
import numpy as np
import torch

U32 = 2.0 ** -24                  # fp32 unit roundoff
ULPS = 16                         # the one-step bar: ULPS * U32 * magnitude (8 ulps of it at most)

MUTATIONS = (
    "mode1_no_cur_sample",        # PLMS warm-up step 1 steps from the current sample instead of the stored one
    "mode1_no_shift",             # PLMS warm-up step 1 without `t += ratio`
    "ets_swap23",                 # fourth-order PLMS with the two oldest history entries swapped
    "final_alpha_one",            # set_alpha_to_one=True
    "euler_dsigma_off_by_one",    # Euler with the next step's sigma difference
    "blend_mask_first",           # background blend with M[0] instead of M[R-1]
    "blend_pre_step_ref",         # background blend from the reference latents before this step
    "xl_le",                      # SDXL: the reference pair is stepped while i <= ibg * n
)


# ---------------------------------------------------------------------------------------------------------- tables
def alphas_cumprod(num_train=1000):
    """scaled_linear betas 0.00085 .. 0.012, cumulative product in fp32 (the table every scheduler here indexes)."""
    betas = torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, num_train, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0)


def plms_timesteps(n, num_train=1000):
    ts = np.arange(0, n) * (num_train // n) + 1
    return [int(t) for t in np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1]]


def euler_schedule(n, num_train=1000):
    """(timesteps float32 [n], sigmas float32 [n+1] ending in 0)."""
    ac = alphas_cumprod(num_train).double().numpy()
    train = ((1 - ac) / ac) ** 0.5
    ts = (np.arange(0, n) * (num_train // n))[::-1].astype(np.float32) + 1
    sig = np.interp(ts, np.arange(0, num_train), train)
    return ts, np.concatenate([sig, [0.0]]).astype(np.float32)


# ---------------------------------------------------------------------------------------------------------- (value, magnitude)
def exact(x):
    return (x, x.abs())


def lin(*terms):
    """sum of c * q over (c, q) terms, c a number or a non-negative mask tensor."""
    v = sum(c * q[0] for c, q in terms)
    m = sum((c.abs() if torch.is_tensor(c) else abs(c)) * q[1] for c, q in terms)
    return v, m


def cfg(u, t, g):
    """u + g * (t - u) in that operation order."""
    return u[0] + g * (t[0] - u[0]), u[1] + abs(g) * (t[1] + u[1])


def cat(*qs):
    return torch.cat([q[0] for q in qs]), torch.cat([q[1] for q in qs])


def rows(q, a, b):
    return q[0][a:b], q[1][a:b]


# ---------------------------------------------------------------------------------------------------------- schedulers
class PLMS:
    """One PLMS sampler over a batch of streams [lat, lat_ref][:S].  The history is per row: when the batch shrinks to the leading row,
    that row keeps its history."""
    kind = 1

    def __init__(self, n, mutations=()):
        self.n_steps, self.mut = n, set(mutations)
        self.timesteps = plms_timesteps(n)
        self.ac = alphas_cumprod().double()
        self.ratio = 1000 // n
        self.ets, self.counter, self.cur = [], 0, None

    def table(self):
        return alphas_cumprod().tolist()

    def step(self, i, eps, x):
        """eps: (value, magnitude) [S,4,h,w]; x: the exact samples [S,4,h,w] -> (value, magnitude) of the new samples."""
        S = x.shape[0]
        t = self.timesteps[i]
        prev_t = t - self.ratio
        if self.counter != 1:
            self.ets = self.ets[-3:] + [eps]
        else:
            prev_t = t
            if "mode1_no_shift" not in self.mut:
                t = t + self.ratio
        e = [rows(q, 0, S) for q in self.ets]
        sample = exact(x)
        if len(e) == 1 and self.counter == 0:
            self.cur = x
            ep = eps
        elif len(e) == 1 and self.counter == 1:
            ep = lin((0.5, eps), (0.5, e[-1]))
            if "mode1_no_cur_sample" not in self.mut:
                sample = exact(self.cur[:S])
        elif len(e) == 2:
            ep = lin((1.5, e[-1]), (-0.5, e[-2]))
        elif len(e) == 3:
            ep = lin((23 / 12, e[-1]), (-16 / 12, e[-2]), (5 / 12, e[-3]))
        else:
            e3, e4 = (e[-4], e[-3]) if "ets_swap23" in self.mut else (e[-3], e[-4])
            ep = lin((55 / 24, e[-1]), (-59 / 24, e[-2]), (37 / 24, e3), (-9 / 24, e4))
        final = 1.0 if "final_alpha_one" in self.mut else self.ac[0].item()
        a_t = self.ac[t].item()
        a_p = self.ac[prev_t].item() if prev_t >= 0 else final
        b_t, b_p = 1 - a_t, 1 - a_p
        ca = (a_p / a_t) ** 0.5
        cb = (a_p - a_t) / (a_t * b_p ** 0.5 + (a_t * b_t * a_p) ** 0.5)
        self.counter += 1
        return lin((ca, sample), (-cb, ep))


class Euler:
    kind = 0

    def __init__(self, n, mutations=()):
        self.n_steps, self.mut = n, set(mutations)
        ts, sig = euler_schedule(n)
        self.timesteps = [float(t) for t in ts]
        self.sig32 = sig
        self.sigmas = [float(s) for s in sig]

    def table(self):
        return self.sigmas

    def step(self, i, eps, x):
        j = i + 1 if "euler_dsigma_off_by_one" in self.mut else i
        ds = self.sigmas[min(j + 1, self.n_steps)] - self.sigmas[j]
        return lin((1.0, exact(x)), (ds, eps))


def make_sched(kind, n, mutations=()):
    return (PLMS if kind == "plms" else Euler)(n, mutations)


# ---------------------------------------------------------------------------------------------------------- the rich-text step
def roles(R):
    return ["u", "b", "ur", "tr"] + [f"r{k}" for k in range(R - 1)]


def plan(i, timesteps, R, isa, ibg, xl, elide=False, mutations=()):
    """Stream list and flags of rich step i: rd.py:99-105 / xl.py:779-783, xl.py:832, rd.py:171 / xl.py:870, and the elision rule.
    `timesteps[j] > (1 - isa) * 1000` compares in float32 as torch does for a tensor element against a Python float."""
    n = len(timesteps)
    use_ref = isa > 0 or ibg > 0
    thr = np.float32((1.0 - isa) * 1000.0)
    feat = [bool(np.float32(t) > thr) for t in timesteps]
    bg_index = int(ibg * n)
    blend = i == bg_index and ibg > 0
    step_ref = use_ref
    if xl:
        step_ref = isa > 0 or (i <= ibg * n if "xl_le" in mutations else i < ibg * n)
    run_ref = use_ref
    if use_ref and elide:
        last_use = max([bg_index if ibg > 0 else -1] + [j for j in range(n) if feat[j]])
        run_ref = i <= last_use
    step_ref = step_ref and run_ref
    streams = ["u", "b"] + (["ur", "tr"] if run_ref else []) + [f"r{k}" for k in range(R - 1)]
    return dict(streams=streams, run_ref=run_ref, step_ref=step_ref, blend=blend, use_ref=use_ref)


def combine(ep, M, g):
    """rd.py:119-132 / xl.py:810-825 + CFG: ep maps a role to its exact [1,4,h,w] prediction, M = R masks [1,4,h,w]."""
    R = len(M)
    nu = lin((M[-1], ep["u"]), *[(M[r], ep["u"]) for r in range(R - 1)])
    nt = lin((M[-1], ep["b"]), *[(M[r], ep[f"r{r}"]) for r in range(R - 1)])
    return cfg(nu, nt, g)


def rich_step(sched, i, ep, M, x, x_ref, g, isa, ibg, xl, elide=False, mutations=()):
    """One rich step from exact (x, x_ref) [1,4,h,w] with exact per-role predictions `ep` -> dict of (value, magnitude): lat, lat_ref,
    noise_pred (the CFG-combined prediction), and the plan."""
    mut = set(mutations)
    p = plan(i, sched.timesteps, len(M), isa, ibg, xl, elide, mut)
    e = combine({k: exact(v) for k, v in ep.items()}, M, g)
    if p["step_ref"]:
        er = cfg(exact(ep["ur"]), exact(ep["tr"]), g)
        out = sched.step(i, cat(e, er), torch.cat([x, x_ref]))
        lat, lat_ref = rows(out, 0, 1), rows(out, 1, 2)
    else:
        lat, lat_ref = sched.step(i, e, x), exact(x_ref)
    if p["blend"]:
        ml = M[0] if "blend_mask_first" in mut else M[-1]
        src = exact(x_ref) if "blend_pre_step_ref" in mut else lat_ref
        lat = lin((ml, src), (1 - ml, lat))
    return dict(lat=lat, lat_ref=lat_ref, noise_pred=e, **p)


def plain_step(sched, i, eu, et, x, g):
    return sched.step(i, cfg(exact(eu), exact(et), g), x)


# ---------------------------------------------------------------------------------------------------------- the test matrix
# (name, scheduler, mode, R, n, latent (h, w), engine (h, w), isa, ibg, elide, defer_blend)
def _c(name, kind, mode, R, n, lat=(32, 32), eng=None, isa=0.0, ibg=0.0, elide=False, defer=False):
    return dict(name=name, kind=kind, mode=mode, R=R, n=n, lat=lat, eng=eng or lat, isa=isa, ibg=ibg, elide=elide, defer=defer,
                xl=kind == "euler", g=5.0 if kind == "euler" else 7.5)


CASES = (
    [_c(f"sd_rich_n{n}", "plms", "rich", 2, n, isa=0.5, ibg=0.3) for n in (1, 2, 3, 4, 5, 10, 50)]
    + [_c("sd_rich_R1_n5", "plms", "rich", 1, 5, isa=0.5, ibg=0.5),
       _c("sd_rich_R13_n10", "plms", "rich", 13, 10, lat=(16, 16), eng=(32, 32), isa=0.5, ibg=0.3),
       _c("sd_rich_24x40_n10", "plms", "rich", 4, 10, lat=(24, 40), eng=(32, 48), isa=0.5, ibg=0.3),
       # the pair stops after step 3 (t > 700 up to step 3, blend at int(0.2 * 11) = 2): mid-way through the PLMS warm-up
       _c("sd_elided_n10", "plms", "rich", 4, 10, isa=0.3, ibg=0.2, elide=True),
       _c("sd_elided_n4_12x8", "plms", "rich", 2, 4, lat=(12, 8), eng=(32, 32), isa=0.0, ibg=0.5, elide=True),
       _c("sd_deferred_n5", "plms", "rich", 3, 5, isa=0.5, ibg=0.5, defer=True),
       _c("sd_deferred_n10_12x8", "plms", "rich", 4, 10, lat=(12, 8), eng=(32, 32), isa=0.0, ibg=0.3, defer=True)]
    + [_c(f"sd_plain_n{n}", "plms", "plain", 0, n) for n in (1, 2, 3, 4, 5, 10, 50)]
    + [_c(f"xl_inject_n{n}", "euler", "rich", 2, n, isa=0.5, ibg=0.3) for n in (1, 2, 3, 10)]
    + [_c("xl_inject_R13_n5", "euler", "rich", 13, 5, lat=(16, 16), eng=(32, 32), isa=0.3, ibg=0.5),
       _c("xl_inject_24x40_n10", "euler", "rich", 4, 10, lat=(24, 40), eng=(32, 48), isa=0.5, ibg=0.3)]
    # isa = 0: the reference pair is stepped while i < ibg * n; 0.14 * 50 = 7.000000000000001, 0.3 * 50 = 15.0, 0.58 * 50 = 28.999999999999996
    + [_c(f"xl_stop_{ibg}_n50", "euler", "rich", R, 50, isa=0.0, ibg=ibg) for ibg, R in ((0.14, 2), (0.3, 4), (0.58, 1))]
    + [_c("xl_stop_0.5_n5_12x8", "euler", "rich", 2, 5, lat=(12, 8), eng=(32, 32), isa=0.0, ibg=0.5),
       _c("xl_stop_0.3_n10_deferred", "euler", "rich", 3, 10, isa=0.0, ibg=0.3, defer=True)]
    + [_c(f"xl_plain_n{n}", "euler", "plain", 0, n) for n in (1, 2, 5, 50)]
    + [_c("xl_plain_n10_24x40", "euler", "plain", 0, 10, lat=(24, 40), eng=(32, 48))]
)
CASE = {c["name"]: c for c in CASES}


def case_inputs(case, seed=0):
    """Seeded fp32 inputs of a case: x_T [1,4,h,w], R masks [1,4,h,w] (a partition of unity over the regions), and per step a
    prediction for every role (the plain step uses "u" and "b")."""
    h, w = case["lat"]
    g = torch.Generator().manual_seed(1000 + 7 * seed + sum(map(ord, case["name"])))
    R = max(case["R"], 1)
    m = torch.softmax(torch.randn(R, 1, h, w, generator=g) * 2, 0).repeat(1, 4, 1, 1)
    sched = make_sched(case["kind"], case["n"])
    scale = (sched.sigmas[0] ** 2 + 1) ** 0.5 if case["kind"] == "euler" else 1.0
    x = torch.randn(1, 4, h, w, generator=g) * scale
    steps = [{k: torch.randn(1, 4, h, w, generator=g) for k in roles(R)} for _ in sched.timesteps]
    return x, [m[r:r + 1] for r in range(R)], steps


def run_restated(case, mutations=(), elide=None):
    """The restatement fed its own output (fp64): the list of (lat, lat_ref) values after every step."""
    x, M, steps = case_inputs(case)
    x, M = x.double(), [m.double() for m in M]
    sched = make_sched(case["kind"], case["n"], mutations)
    lat, lat_ref, out = x, x.clone(), []
    for i, ep in enumerate(steps):
        ep = {k: v.double() for k, v in ep.items()}
        if case["mode"] == "plain":
            lat = plain_step(sched, i, ep["u"], ep["b"], lat, case["g"])[0]
        else:
            r = rich_step(sched, i, ep, M, lat, lat_ref, case["g"], case["isa"], case["ibg"], case["xl"],
                          case["elide"] if elide is None else elide, mutations)
            lat, lat_ref = r["lat"][0], r["lat_ref"][0]
        out.append((lat, lat_ref))
    return out


def one_step_margins(case, mutations):
    """Largest max|mutated - unmutated| / max(bar) over every one-step output of the case, both stepped from the unmutated trajectory
    (the bar of the whole tensor: an elementwise ratio would be inflated wherever the magnitude happens to be small)."""
    x, M, steps = case_inputs(case)
    x, M = x.double(), [m.double() for m in M]
    good, bad = make_sched(case["kind"], case["n"]), make_sched(case["kind"], case["n"], mutations)
    lat, lat_ref, worst = x, x.clone(), 0.0
    for i, ep in enumerate(steps):
        ep = {k: v.double() for k, v in ep.items()}
        if case["mode"] == "plain":
            ra = plain_step(good, i, ep["u"], ep["b"], lat, case["g"])
            rb = plain_step(bad, i, ep["u"], ep["b"], lat, case["g"])
            pairs, lat = [(ra, rb)], ra[0]
        else:
            a = rich_step(good, i, ep, M, lat, lat_ref, case["g"], case["isa"], case["ibg"], case["xl"], case["elide"])
            b = rich_step(bad, i, ep, M, lat, lat_ref, case["g"], case["isa"], case["ibg"], case["xl"], case["elide"], mutations)
            pairs = [(a["lat"], b["lat"]), (a["lat_ref"], b["lat_ref"])]
            lat, lat_ref = a["lat"][0], a["lat_ref"][0]
        for ra, rb in pairs:
            worst = max(worst, (ra[0] - rb[0]).abs().max().item() / (ULPS * U32 * ra[1].max().item()))
    return worst
