"""Host-side scheduler tables for the engine (product code; the oracle keeps an independent copy).

Restates the published diffusers 0.18.2 `PNDMScheduler` (skip_prk_steps=True, steps_offset=1; used at
models/region_diffusion.py:35-37), `EulerDiscreteScheduler` (SDXL config; models/region_diffusion_sdxl.py:120) and
`DPMSolverMultistepScheduler` (dpmsolver++, midpoint, epsilon, lower_order_final; imported at models/region_diffusion.py:7, never
wired in there).
Only the *tables* live here (timesteps, sigmas, alphas_cumprod); the update arithmetic runs in
csrc/step.hip.  diffusers is third-party and not on disk => [memory], parity unpinned."""
import numpy as np
import torch


def alphas_cumprod(num_train=1000, beta_start=0.00085, beta_end=0.012):
    # fp32 torch arithmetic, as diffusers builds the "scaled_linear" schedule
    betas = torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train, dtype=torch.float32) ** 2
    return torch.cumprod(1.0 - betas, dim=0).numpy()


class PNDMTables:
    kind = 1
    init_noise_sigma = 1.0

    def __init__(self, num_train=1000):
        self.num_train = num_train
        self.alphas_cumprod = alphas_cumprod(num_train)

    def set_timesteps(self, n):
        self.num_inference_steps = n
        ts = (np.arange(0, n) * (self.num_train // n)).round() + 1
        self.timesteps = np.concatenate([ts[:-1], ts[-2:-1], ts[-1:]])[::-1].astype(np.int64).copy()
        return self

    def table(self):
        return self.alphas_cumprod.tolist()


class EulerTables:
    kind = 0

    def __init__(self, num_train=1000):
        self.num_train = num_train
        ac = alphas_cumprod(num_train).astype(np.float64)
        self.alphas_cumprod = alphas_cumprod(num_train)
        self._train_sigmas = ((1 - ac) / ac) ** 0.5
        self.init_noise_sigma = float(self._train_sigmas.max())

    def set_timesteps(self, n):
        self.num_inference_steps = n
        ts = (np.arange(0, n) * (self.num_train // n)).round()[::-1].copy().astype(np.float32) + 1
        sig = np.interp(ts, np.arange(0, self.num_train), self._train_sigmas)
        self.sigmas = np.concatenate([sig, [0.0]]).astype(np.float32)
        self.timesteps = ts
        self.init_noise_sigma = float((self.sigmas.max() ** 2 + 1) ** 0.5)
        return self

    def table(self):
        return self.sigmas.tolist()


class DPMSolverTables:
    """DPM-Solver++(1M / 2M), either pipeline: `pipe.scheduler = DPMSolverTables()`.  `table()` is alphas_cumprod: the engine derives
    alpha / sigma / lambda from it and keeps each stream's x0 history itself (rt_set_schedule resets it)."""
    init_noise_sigma = 1.0

    def __init__(self, solver_order=2, num_train=1000):
        if solver_order not in (1, 2):
            raise ValueError(f"DPMSolverTables: solver_order must be 1 or 2, got {solver_order}")
        self.solver_order = solver_order
        self.kind = 3 if solver_order == 2 else 2                      # RT_SCHED_DPMPP_2 / RT_SCHED_DPMPP_1
        self.num_train = num_train
        self.alphas_cumprod = alphas_cumprod(num_train)
        ac = torch.from_numpy(self.alphas_cumprod)
        self.alpha_t = torch.sqrt(ac)
        self.sigma_t = torch.sqrt(1 - ac)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)

    def set_timesteps(self, n):
        ts = np.linspace(0, self.num_train - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        _, first = np.unique(ts, return_index=True)
        self.timesteps = ts[np.sort(first)]
        self.num_inference_steps = len(self.timesteps)
        return self

    def table(self):
        return self.alphas_cumprod.tolist()
