"""Test helper (not collected): DPM-Solver++ multistep restated for the tests, independently of the product's schedulers.py and
csrc/step_driver.inl.

[memory] diffusers 0.18.2 `DPMSolverMultistepScheduler` with algorithm_type="dpmsolver++", solver_type="midpoint",
prediction_type="epsilon", lower_order_final=True, no thresholding, no Karras sigmas, lambda_min_clipped=-inf, solver_order 1 or 2.
diffusers is not on disk, so parity against it is UNPINNED (like PNDM / Euler in oracle/schedulers.py); the CPU tests pin the
arithmetic against the mathematics instead (DDIM identity, convergence order on an analytic probability-flow ODE).

History is per stream: `RefDPMSolver.step` keeps one x0 per batch row.  When the batch shrinks (the rich-text loops stop stepping the
reference pair: cat([lat, lat_ref]) -> lat), the leading rows keep their history and the dropped rows' history is no longer used.
"""
import numpy as np
import torch

from oracle.schedulers import scaled_linear_alphas_cumprod


def dpm_timesteps(n, num_train=1000):
    ts = np.linspace(0, num_train - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
    _, idx = np.unique(ts, return_index=True)
    return ts[np.sort(idx)]


def dpm_tables(dtype=torch.float32, num_train=1000):
    """(alphas_cumprod, alpha, sigma, lambda) - fp32 torch arithmetic on the fp32 scaled-linear table, or `dtype` throughout."""
    ac = scaled_linear_alphas_cumprod(num_train).to(dtype)
    alpha = torch.sqrt(ac)
    sigma = torch.sqrt(1 - ac)
    lam = torch.log(alpha) - torch.log(sigma)
    return ac, alpha, sigma, lam


def dpm_update(x, x0, s0, p, alpha, sigma, lam, s1=None, m1=None):
    """One DPM-Solver++ update from timestep s0 to p: first order without (s1, m1), second order (midpoint) with them."""
    h = lam[p] - lam[s0]
    c1 = alpha[p] * (torch.exp(-h) - 1.0)
    out = (sigma[p] / sigma[s0]) * x - c1 * x0
    if m1 is None:
        return out
    r0 = (lam[s0] - lam[s1]) / h
    d1 = (1.0 / r0) * (x0 - m1)
    return out - 0.5 * c1 * d1


class RefDPMSolver:
    """The scheduler surface the oracle loops touch (set_timesteps / timesteps / step / scale_model_input / alphas_cumprod /
    init_noise_sigma), with per-stream (per batch row) history."""
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, solver_order=2, dtype=torch.float32):
        assert solver_order in (1, 2)
        self.solver_order = solver_order
        self.alphas_cumprod, self.alpha_t, self.sigma_t, self.lambda_t = dpm_tables(dtype)
        self.dtype = dtype

    def set_timesteps(self, n, device=None):
        self.timesteps = torch.from_numpy(dpm_timesteps(n))
        self.num_inference_steps = len(self.timesteps)
        self.m1 = None                  # x0 of the previous step, one row per stream
        self.prev_t = None
        self.lower_order_nums = 0
        self.step_index = 0
        return self

    def scale_model_input(self, sample, t=None):
        return sample

    def step(self, model_output, timestep, sample, return_dict=True, **kw):
        ts = self.timesteps.tolist()
        i = ts.index(int(timestep))
        assert i == self.step_index, "RefDPMSolver: steps must come in schedule order"
        n = len(ts)
        s0, p = ts[i], (0 if i == n - 1 else ts[i + 1])
        a, s, lam = self.alpha_t, self.sigma_t, self.lambda_t
        x0 = (sample - s[s0] * model_output) / a[s0]
        lower_final = i == n - 1 and n < 15
        if self.solver_order == 1 or self.lower_order_nums < 1 or lower_final:
            prev = dpm_update(sample, x0, s0, p, a, s, lam)
        else:
            m1 = self.m1[:sample.shape[0]]
            prev = dpm_update(sample, x0, s0, p, a, s, lam, s1=self.prev_t, m1=m1)
        if self.m1 is None or self.m1.shape[0] <= x0.shape[0]:
            self.m1 = x0
        else:                            # shrinking batch: the stopped streams keep their (unused) history
            self.m1 = torch.cat([x0, self.m1[x0.shape[0]:]])
        self.prev_t = s0
        self.lower_order_nums = min(self.lower_order_nums + 1, self.solver_order)
        self.step_index += 1
        return {"prev_sample": prev} if return_dict else (prev,)
