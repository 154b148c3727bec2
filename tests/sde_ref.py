"""Test helper (not collected): the stochastic samplers restated for the tests, independently of the product's schedulers.py,
csrc/philox.h and csrc/step_driver.inl.

  * The noise field: Philox4x32-10 (Random123: multipliers D2511F53 / CD9E8D57, Weyl constants 9E3779B9 / BB67AE85, ten rounds) in numpy
    uint64 arithmetic, key = (seed & 0xffffffff, seed >> 32), counter = (pixel, step, 0, 0); the four words of a pixel give its four
    channels by Box-Muller in fp64: u1 = ((r0 >> 8) + 1) 2^-24, u2 = (r1 >> 8) 2^-24, rad = sqrt(-2 ln u1), (rad cos 2 pi u2,
    rad sin 2 pi u2); channels 2 / 3 from (r2, r3).
  * RefEulerAncestral / RefSdeDpmSolver: [memory] diffusers' EulerAncestralDiscreteScheduler (SDXL config: leading spacing, steps_offset
    1, epsilon) and DPMSolverMultistepScheduler with algorithm_type="sde-dpmsolver++" (midpoint, epsilon, lower_order_final), with the
    set_timesteps / scale_model_input / step(...)["prev_sample"] surface of tests/dpm_solver_ref.py.  diffusers is not on disk: parity is
    UNPINNED; tests/test_stochastic.py pins the arithmetic to the point-mass identities instead.
    The noise comes from `noise_fn(i)` -> [1,4,h,w], i = the index of the step in the EXECUTED schedule; the same field goes to every
    row of a batched step.  History is per row, as in RefDPMSolver.  `strength` < 1 runs the last min(int(n strength), n) steps.
"""
import numpy as np
import torch

from oracle.schedulers import scaled_linear_alphas_cumprod

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four uint64 arrays (values < 2^32) or ints, key: two ints -> four uint64 arrays of 32-bit words."""
    c = [np.asarray(v, dtype=np.uint64) & np.uint64(MASK) for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & MASK, int(key[1]) & MASK
    m = np.uint64(MASK)
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]                      # < 2^64: exact in uint64
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & m, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & m]
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c


def noise_words(seed, step, npix):
    """[npix, 4] uint64: the Philox words of pixels 0 .. npix-1 at `step`."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    r = philox4x32_10((np.arange(npix, dtype=np.uint64), int(step), 0, 0), (seed & MASK, seed >> 32))
    return np.stack(r, axis=1)


def normals_from_words(words):
    """words [npix, 4] -> (z [npix, 4] fp64, rad [npix, 4] fp64: the Box-Muller radius each value was scaled by)."""
    w = words.astype(np.uint64)
    z, rad = np.empty(w.shape, dtype=np.float64), np.empty(w.shape, dtype=np.float64)
    for a in (0, 2):
        u1 = ((w[:, a] >> np.uint64(8)).astype(np.float64) + 1.0) * 2.0 ** -24
        u2 = (w[:, a + 1] >> np.uint64(8)).astype(np.float64) * 2.0 ** -24
        r = np.sqrt(-2.0 * np.log(u1))
        z[:, a], z[:, a + 1] = r * np.cos(2.0 * np.pi * u2), r * np.sin(2.0 * np.pi * u2)
        rad[:, a] = rad[:, a + 1] = r
    return z, rad


def noise_field(seed, step, h, w):
    """(z, rad) as fp64 arrays [4, h, w]: pixel y * w + x, channel c."""
    z, rad = normals_from_words(noise_words(seed, step, h * w))
    return z.T.reshape(4, h, w).copy(), rad.T.reshape(4, h, w).copy()


def field_fn(seed, h, w, dtype=torch.float64):
    """noise_fn of the restated field itself (CPU tests)."""
    return lambda i: torch.from_numpy(noise_field(seed, i, h, w)[0])[None].to(dtype)


def executed_steps(n, strength):
    assert 0.0 < strength <= 1.0
    k = min(int(n * strength), n)
    assert k >= 1
    return k


def vp_level(ac, t):
    a = float(ac[int(t)])
    return a ** 0.5, (1.0 - a) ** 0.5


class RefEulerAncestral:
    order = 1

    def __init__(self, noise_fn, dtype=torch.float32, strength=1.0, num_train=1000):
        self.noise_fn, self.dtype, self.strength, self.num_train = noise_fn, dtype, strength, num_train
        self.alphas_cumprod = scaled_linear_alphas_cumprod(num_train)
        ac = self.alphas_cumprod.double().numpy()
        self._train_sigmas = ((1 - ac) / ac) ** 0.5

    def set_timesteps(self, n, device=None):
        k = executed_steps(n, self.strength)
        ts = (np.arange(0, n) * (self.num_train // n))[::-1].astype(np.float32) + 1
        sig = np.concatenate([np.interp(ts, np.arange(0, self.num_train), self._train_sigmas), [0.0]]).astype(np.float32)
        self.init_noise_sigma = float((sig.max() ** 2 + 1) ** 0.5)
        self.timesteps = torch.from_numpy(ts[n - k:].copy())
        self.sigmas = torch.from_numpy(sig[n - k:].copy())
        self.num_inference_steps = n
        self.step_index = 0
        return self

    def _index(self, t):
        return self.timesteps.tolist().index(float(t))

    def scale_model_input(self, sample, t):
        s = self.sigmas[self._index(t)].to(self.dtype)
        return sample / ((s ** 2 + 1) ** 0.5)

    def start_level(self):
        return 1.0, float(self.sigmas[0])

    def source_levels(self):
        return [(1.0, float(s)) for s in self.sigmas[1:-1]] + [(1.0, 0.0)]

    def coefficients(self, i):
        s, sp = self.sigmas[i].to(self.dtype), self.sigmas[i + 1].to(self.dtype)
        up = torch.sqrt(sp * sp * (s * s - sp * sp) / (s * s))
        down = torch.sqrt(sp * sp - up * up)
        return s, sp, up, down

    def step(self, model_output, timestep, sample, return_dict=True, **kw):
        i = self._index(timestep)
        assert i == self.step_index, "RefEulerAncestral: steps must come in schedule order"
        s, sp, up, down = self.coefficients(i)
        z = self.noise_fn(i).to(self.dtype)
        prev = sample + model_output * (down - s) + z * up
        self.step_index += 1
        return {"prev_sample": prev} if return_dict else (prev,)


class RefSdeDpmSolver:
    order = 1
    init_noise_sigma = 1.0

    def __init__(self, noise_fn, solver_order=2, dtype=torch.float32, strength=1.0, num_train=1000):
        assert solver_order in (1, 2)
        self.noise_fn, self.solver_order, self.dtype, self.strength, self.num_train = noise_fn, solver_order, dtype, strength, num_train
        self.alphas_cumprod = scaled_linear_alphas_cumprod(num_train)
        ac = self.alphas_cumprod.to(dtype)
        self.alpha_t = torch.sqrt(ac)
        self.sigma_t = torch.sqrt(1 - ac)
        self.lambda_t = torch.log(self.alpha_t) - torch.log(self.sigma_t)

    def set_timesteps(self, n, device=None):
        k = executed_steps(n, self.strength)
        ts = np.linspace(0, self.num_train - 1, n + 1).round()[::-1][:-1].copy().astype(np.int64)
        _, idx = np.unique(ts, return_index=True)
        ts = ts[np.sort(idx)]
        if k < n:
            ts = ts[n - k:]
        assert len(ts) >= 1
        self.timesteps = torch.from_numpy(ts.copy())
        self.num_inference_steps = len(ts)
        self.m1, self.prev_t, self.lower_order_nums, self.step_index = None, None, 0, 0
        return self

    def scale_model_input(self, sample, t=None):
        return sample

    def start_level(self):
        return vp_level(self.alphas_cumprod, self.timesteps[0])

    def source_levels(self):
        return [vp_level(self.alphas_cumprod, t) for t in self.timesteps[1:]] + [(1.0, 0.0)]

    def step(self, model_output, timestep, sample, return_dict=True, **kw):
        ts = self.timesteps.tolist()
        i = ts.index(int(timestep))
        assert i == self.step_index, "RefSdeDpmSolver: steps must come in schedule order"
        n = len(ts)
        s0, p = ts[i], (0 if i == n - 1 else ts[i + 1])
        a, s, lam = self.alpha_t, self.sigma_t, self.lambda_t
        x0 = (sample - s[s0] * model_output) / a[s0]
        h = lam[p] - lam[s0]
        q = 1.0 - torch.exp(-2.0 * h)
        prev = (s[p] / s[s0] * torch.exp(-h)) * sample + (a[p] * q) * x0
        lower_final = i == n - 1 and n < 15
        if not (self.solver_order == 1 or self.lower_order_nums < 1 or lower_final):
            r0 = (lam[s0] - lam[self.prev_t]) / h
            prev = prev + (0.5 * (a[p] * q)) * ((1.0 / r0) * (x0 - self.m1[:sample.shape[0]]))
        prev = prev + (s[p] * torch.sqrt(q)) * self.noise_fn(i).to(self.dtype)
        if self.m1 is None or self.m1.shape[0] <= x0.shape[0]:
            self.m1 = x0
        else:                            # shrinking batch: the stopped streams keep their (unused) history
            self.m1 = torch.cat([x0, self.m1[x0.shape[0]:]])
        self.prev_t = s0
        self.lower_order_nums = min(self.lower_order_nums + 1, self.solver_order)
        self.step_index += 1
        return {"prev_sample": prev} if return_dict else (prev,)
