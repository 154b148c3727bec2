"""Host-side scheduler tables for the engine (product code; the oracle keeps an independent copy).

Restates the published diffusers 0.18.2 `PNDMScheduler` (skip_prk_steps=True, steps_offset=1; used at
models/region_diffusion.py:35-37), `EulerDiscreteScheduler` (SDXL config; models/region_diffusion_sdxl.py:120) and
`DPMSolverMultistepScheduler` (dpmsolver++, midpoint, epsilon, lower_order_final; imported at models/region_diffusion.py:7, never
wired in there), and the two stochastic samplers that share their tables: `EulerAncestralDiscreteScheduler` and
`DPMSolverMultistepScheduler` with algorithm_type="sde-dpmsolver++" (their noise is made by the engine: Engine.set_noise_seed).
Only the *tables* live here (timesteps, sigmas, alphas_cumprod); the update arithmetic runs in
csrc/step.hip.  diffusers is third-party and not on disk => [memory], parity unpinned."""
import numpy as np
import torch


def alphas_cumprod(num_train=1000, beta_start=0.00085, beta_end=0.012):
    # fp32 torch arithmetic, as diffusers builds the "scaled_linear" schedule
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).numpy()


# ---- starting from an image (`set_timesteps(n, strength)`) --------------------------------------------------------------------------
# strength in (0, 1]: the last k = min(int(n * strength), n) solver steps of the n-step schedule are executed, t_start = n - k.  The
# truncated lists go to rt_set_schedule as they are, so `inject_background` is a fraction of the EXECUTED schedule, while
# `inject_selfattn` keeps its timestep threshold (t > (1 - inject_selfattn) * 1000) whatever the strength.
#   start_level()   -> (a, b): the loop starts from a * x0 + b * noise
#   source_levels() -> one (a, b) per loop iteration: the level the latents are at AFTER it (what a pinned pixel is reset to);
#                      the last one is (1, 0) for every scheduler: a pinned pixel ends as the source itself.
PREDICTION_TYPES = ('epsilon', 'v_prediction')
TIMESTEP_SPACINGS = ('leading', 'trailing')


def check_prediction_type(v, who='prediction_type'):
    if v not in PREDICTION_TYPES:
        raise ValueError(f"{who} must be one of {PREDICTION_TYPES}, got {v!r}")
    return v


def _check_spacing(name, v):
    if v not in TIMESTEP_SPACINGS:
        raise ValueError(f"{name}: timestep_spacing must be one of {TIMESTEP_SPACINGS}, got {v!r}")
    return v


def trailing_timesteps(n, num_train=1000):
    """round(num_train - k num_train / n) - 1 for k = 0 .. n-1 ([memory]: diffusers' timestep_spacing="trailing"; the first step is the
    last training timestep, which is what zero-terminal-SNR / v-prediction checkpoints are sampled with)."""
    return (np.round(num_train - np.arange(n) * (num_train / n)) - 1).astype(np.int64)


def engine_prediction(scheduler, guidance_scale, call_rescale=0.0, pipeline_rescale=0.0):
    """(prediction_type, phi) for Engine.set_prediction: the scheduler's `prediction_type` attribute; phi = the call's guidance_rescale
    if > 0, else the pipeline's, and only under classifier-free guidance (guidance_scale > 1, xl.py:903)."""
    ptype = check_prediction_type(getattr(scheduler, 'prediction_type', 'epsilon'), f"{type(scheduler).__name__}.prediction_type")
    phi = float(call_rescale) if call_rescale and call_rescale > 0 else float(pipeline_rescale or 0.0)
    if not (0.0 <= phi <= 1.0):
        raise ValueError(f"guidance_rescale must be in [0, 1], got {phi}")
    return ptype, (phi if guidance_scale > 1.0 else 0.0)


def _executed_steps(name, n, strength, least=1):
    if not (0.0 < strength <= 1.0):
        raise ValueError(f"{name}.set_timesteps: strength must be in (0, 1], got {strength}")
    k = min(int(n * strength), n)
    if k < least:
        raise ValueError(f"{name}.set_timesteps: strength {strength} of {n} steps leaves {k} solver steps, need at least {least}")
    return k


def _vp_level(ac, t):
    a = float(ac[int(t)])                         # fp64 arithmetic on the fp32 table entry
    return a ** 0.5, (1.0 - a) ** 0.5


class PNDMTables:
    kind = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train=1000, prediction_type='epsilon', timestep_spacing='leading'):
        """`prediction_type` is an attribute the pipelines hand to the engine (Engine.set_prediction): the tables do not depend on it.
        PLMS's `prev_t = t - num_train // n` arithmetic is leading-only: trailing spacing is refused."""
        self.num_train = num_train
        self.prediction_type = check_prediction_type(prediction_type, "PNDMTables: prediction_type")
        if _check_spacing("PNDMTables", timestep_spacing) != 'leading':
            raise ValueError("PNDMTables: timestep_spacing='trailing' is not supported (the PLMS step assumes t - num_train // n)")
        self.timestep_spacing = timestep_spacing
        self.alphas_cumprod = alphas_cumprod(num_train)

    def set_timesteps(self, n, strength=1.0):
        """strength < 1: the distinct descending timesteps D of the n-step schedule are cut to D[n - k:] and expanded again as PLMS
        expects, [d0, d1, d1, d2, ...] = k + 1 iterations, so the warm-up pair restarts at the cut.  (diffusers' img2img pipelines
        slice the EXPANDED list instead, after which the warm-up leaves every later iteration one timestep behind; this is a deliberate
        deviation, [memory], parity unpinned.)  `num_inference_steps` stays n: the engine's step ratio is 1000 // n."""
        k = _executed_steps("PNDMTables", n, strength, least=min(2, n))
        self.num_inference_steps = n
        ts = (np.arange(0, n) * (self.num_train // n)).round() + 1
        ts = ts[:k]                                # ascending: the k smallest = the last k of the descending list
        self.timesteps = np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].astype(np.int64).copy()
        return self

    def start_level(self):
        return _vp_level(self.alphas_cumprod, self.timesteps[0])

    def source_levels(self):
        """Iterations 0 and 1 (the PLMS warm-up pair) both land on d1, iteration j >= 2 on d_j, the last one on the source."""
        d = [int(self.timesteps[0])] + [int(t) for t in self.timesteps[2:]]            # the distinct list d0, d1, ...
        lands = [d[1]] + d[1:]
        return [_vp_level(self.alphas_cumprod, t) for t in lands] + [(1.0, 0.0)]

    def table(self):
        return self.alphas_cumprod.tolist()


class EulerTables:
    kind = 0

    def __init__(self, num_train=1000, prediction_type='epsilon', timestep_spacing='leading'):
        """`prediction_type`: an attribute for Engine.set_prediction, the tables do not depend on it.  timestep_spacing='trailing':
        trailing_timesteps() instead of the SDXL config's leading list with steps_offset 1."""
        self.num_train = num_train
        self.prediction_type = check_prediction_type(prediction_type, f"{type(self).__name__}: prediction_type")
        self.timestep_spacing = _check_spacing(type(self).__name__, timestep_spacing)
        ac = alphas_cumprod(num_train).astype(np.float64)
        self.alphas_cumprod = alphas_cumprod(num_train)
        self._train_sigmas = ((1 - ac) / ac) ** 0.5
        self.init_noise_sigma = float(self._train_sigmas.max())

    def set_timesteps(self, n, strength=1.0):
        """strength < 1: timesteps and sigmas lose their first n - k entries (the sigmas still end in 0); init_noise_sigma stays the
        full schedule's (an image start does not use it: start_level())."""
        k = _executed_steps("EulerTables", n, strength)
        self.num_inference_steps = n
        if self.timestep_spacing == 'trailing':
            ts = trailing_timesteps(n, self.num_train).astype(np.float32)
        else:
            ts = (np.arange(0, n) * (self.num_train // n)).round()[::-1].copy().astype(np.float32) + 1
        sig = np.interp(ts, np.arange(0, self.num_train), self._train_sigmas)
        self.sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.timesteps = ts
        self.init_noise_sigma = float((self.sigmas.max() ** 2 + 1) ** 0.5)
        if k < n:
            self.timesteps, self.sigmas = self.timesteps[n - k:], self.sigmas[n - k:]
        return self

    def start_level(self):
        return 1.0, float(self.sigmas[0])           # diffusers' Euler add_noise: x0 + sigma * noise

    def source_levels(self):
        return [(1.0, float(s)) for s in self.sigmas[1:-1]] + [(1.0, 0.0)]

    def table(self):
        return self.sigmas.tolist()


class EulerAncestralTables(EulerTables):
    """Euler ancestral ("Euler a"), SDXL family: Euler's timesteps, sigmas and input scaling; each step lands on the level its
    deterministic parent lands on (sigma_down^2 + sigma_up^2 = sigma_{i+1}^2), so start_level() / source_levels() are inherited."""
    kind = 4                                                           # RT_SCHED_EULER_A


class DPMSolverTables:
    """DPM-Solver++(1M / 2M), either pipeline: `pipe.scheduler = DPMSolverTables()`.  `table()` is alphas_cumprod: the engine derives
    alpha / sigma / lambda from it and keeps each stream's x0 history itself (rt_set_schedule resets it).
    algorithm='sde-dpmsolver++': the stochastic variant ("DPM++ 2M SDE") on the same tables, levels and history."""
    init_noise_sigma = 1.0

    def __init__(self, solver_order=2, num_train=1000, algorithm='dpmsolver++', prediction_type='epsilon', timestep_spacing='leading'):
        """`prediction_type`: an attribute for Engine.set_prediction, the tables do not depend on it.  timestep_spacing: 'leading' names
        today's list (diffusers 0.18.2's linspace over [0, num_train - 1]); 'trailing': trailing_timesteps()."""
        self.prediction_type = check_prediction_type(prediction_type, "DPMSolverTables: prediction_type")
        self.timestep_spacing = _check_spacing("DPMSolverTables", timestep_spacing)
        if solver_order not in (1, 2):
            raise ValueError(f"DPMSolverTables: solver_order must be 1 or 2, got {solver_order}")
        if algorithm not in ('dpmsolver++', 'sde-dpmsolver++'):
            raise ValueError(f"DPMSolverTables: algorithm must be 'dpmsolver++' or 'sde-dpmsolver++', got {algorithm!r}")
        self.solver_order = solver_order
        self.algorithm = algorithm
        if algorithm == 'dpmsolver++':
            self.kind = 3 if solver_order == 2 else 2                  # RT_SCHED_DPMPP_2 / RT_SCHED_DPMPP_1
        else:
            self.kind = 6 if solver_order == 2 else 5                  # RT_SCHED_DPMPP_SDE_2 / RT_SCHED_DPMPP_SDE_1
        self.num_train = num_train
        self.alphas_cumprod = alphas_cumprod(num_train)
        ac = torch.from_numpy(self.alphas_cumprod)
        self.alpha_t = torch.sqrt(ac)
        self.sigma_t = torch.sqrt(1 - ac)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)

    def set_timesteps(self, n, strength=1.0):
        """strength < 1: the (de-duplicated) list loses its first n - k entries.  The engine counts `lower_order_final` (a first-order
        last step when fewer than 15 steps run) on the EXECUTED list, where diffusers' img2img counts the full one: a deliberate
        deviation, [memory], parity unpinned."""
        k = _executed_steps("DPMSolverTables", n, strength)
        if self.timestep_spacing == 'trailing':
            ts = trailing_timesteps(n, self.num_train)
        else:
            ts = np.linspace(0, self.num_train - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        _, first = np.unique(ts, return_index=True)
        self.timesteps = ts[np.sort(first)]
        if k < n:
            self.timesteps = self.timesteps[n - k:]
            if len(self.timesteps) == 0:
                raise ValueError(f"DPMSolverTables.set_timesteps: strength {strength} of {n} steps leaves no solver step")
        self.num_inference_steps = len(self.timesteps)
        return self

    def start_level(self):
        return _vp_level(self.alphas_cumprod, self.timesteps[0])

    def source_levels(self):
        return [_vp_level(self.alphas_cumprod, t) for t in self.timesteps[1:]] + [(1.0, 0.0)]

    def table(self):
        return self.alphas_cumprod.tolist()
