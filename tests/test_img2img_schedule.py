"""Truncated schedules of the image start (schedulers.py `set_timesteps(n, strength)`, `start_level()`, `source_levels()`) on the CPU:
against the restatement in tests/img2img_ref.py over an (n, strength) grid, and through an identity that ties the start level to the
tables."""
import numpy as np
import pytest
import torch

from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerTables, PNDMTables
from tests.img2img_ref import dpm_loop, euler_loop, plms_loop, ref_schedule

NS = (4, 10, 20, 41, 50)
STRENGTHS = (0.05, 0.3, 0.5, 0.8, 1.0)
KINDS = {"euler": EulerTables, "pndm": PNDMTables, "dpm": DPMSolverTables}
# the oracle builds Euler's sigmas from an fp32 table, the product from an fp64 one, both rounded to fp32 at the end: two fp32 ulps
SIGMA_RTOL = 2 * 2.0 ** -23


def _k(n, strength):
    return min(int(n * strength), n)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", NS)
def test_strength_one_reproduces_todays_tables(kind, n):
    a, b = KINDS[kind]().set_timesteps(n), KINDS[kind]().set_timesteps(n, strength=1.0)
    assert sorted(vars(a)) == sorted(vars(b))
    for name, va in vars(a).items():
        vb = getattr(b, name)
        if isinstance(va, (np.ndarray, torch.Tensor)):
            assert type(va) is type(vb) and va.dtype == vb.dtype and va.shape == vb.shape, name
            assert np.array_equal(np.asarray(va), np.asarray(vb)), name
        else:
            assert va == vb, name
    # ... and today's tables are the oracle's full ones
    r = ref_schedule(kind, n, 1.0)
    assert np.array_equal(np.asarray(a.timesteps, dtype=np.float64), np.asarray(r["timesteps"], dtype=np.float64))
    if kind == "euler":
        assert np.allclose(a.sigmas, r["sigmas"], rtol=SIGMA_RTOL, atol=0)


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("strength", STRENGTHS)
@pytest.mark.parametrize("n", NS)
def test_truncated_tables_over_the_grid(kind, n, strength):
    k = _k(n, strength)
    t = KINDS[kind]()
    if k == 0 or (kind == "pndm" and k < 2):
        with pytest.raises(ValueError):
            t.set_timesteps(n, strength)
        with pytest.raises(ValueError):
            ref_schedule(kind, n, strength)
        return
    t.set_timesteps(n, strength)
    full = KINDS[kind]().set_timesteps(n)
    r = ref_schedule(kind, n, strength)
    ts = np.asarray(t.timesteps)
    assert np.array_equal(ts.astype(np.float64), np.asarray(r["timesteps"], dtype=np.float64))
    assert ts.dtype == np.asarray(full.timesteps).dtype
    if kind == "euler":
        assert len(ts) == k and len(t.sigmas) == k + 1
        assert np.allclose(t.sigmas, r["sigmas"], rtol=SIGMA_RTOL, atol=0) and t.sigmas[-1] == 0.0 and t.sigmas.dtype == np.float32
        assert np.array_equal(ts, full.timesteps[n - k:]) and np.array_equal(t.sigmas, full.sigmas[n - k:])
        assert t.num_inference_steps == n
    elif kind == "pndm":
        assert len(ts) == k + 1
        D = sorted(set(int(v) for v in full.timesteps), reverse=True)          # the full distinct list
        d = [int(ts[0])] + [int(v) for v in ts[2:]]
        assert d == D[n - k:] and ts[1] == ts[2] == d[1]                        # [d0, d1, d1, d2, ...] drawn from it
        assert t.num_inference_steps == n                                      # the engine's step ratio stays 1000 // n
    else:
        assert 1 <= len(ts) <= k and np.array_equal(ts, full.timesteps[n - k:])
        assert t.num_inference_steps == len(ts)
        assert all(ts[i] > ts[i + 1] for i in range(len(ts) - 1))
    # levels
    rel = SIGMA_RTOL if kind == "euler" else 1e-12
    a, b = t.start_level()
    assert (a, b) == pytest.approx(r["start"], rel=rel, abs=0)
    lv = t.source_levels()
    assert len(lv) == len(ts) == len(r["levels"])
    assert tuple(lv[-1]) == (1.0, 0.0)
    for got, want in zip(lv, r["levels"]):
        assert tuple(got) == pytest.approx(want, rel=rel, abs=0)
    if kind == "euler":
        assert a == 1.0 and b == float(t.sigmas[0]) and all(x[0] == 1.0 for x in lv)
    else:
        for x in [(a, b)] + lv:
            assert x[0] ** 2 + x[1] ** 2 == pytest.approx(1.0, abs=1e-12)       # variance preserving
    if kind == "pndm":
        assert lv[0] == lv[1]                                                   # the warm-up pair lands on d1 twice


@pytest.mark.parametrize("kind", list(KINDS))
def test_error_cases(kind):
    for bad in (0.0, -0.1, 1.0001, 2.0, float("nan")):
        with pytest.raises(ValueError):
            KINDS[kind]().set_timesteps(20, bad)
    with pytest.raises(ValueError):
        KINDS[kind]().set_timesteps(10, 0.05)          # k == 0
    if kind == "pndm":
        with pytest.raises(ValueError):
            PNDMTables().set_timesteps(20, 0.05)       # k == 1: PLMS needs its warm-up pair
    else:
        assert len(KINDS[kind]().set_timesteps(20, 0.05).timesteps) == 1


def _point_mass_run(kind, n, strength, start=None, order=2):
    """The fp64 loop of `kind` on the PRODUCT's tables, started from start_level() (or `start`), with the exact noise prediction of a
    point mass at x0.  -> (x0, noise, final x, trace, levels)"""
    t = KINDS[kind]().set_timesteps(n, strength)
    g = torch.Generator().manual_seed(7)
    x0 = torch.randn(1, 4, 16, 16, generator=g, dtype=torch.float64)
    noise = torch.randn(1, 4, 16, 16, generator=g, dtype=torch.float64)
    a, b = start or t.start_level()
    x = a * x0 + b * noise
    ac = np.asarray(t.alphas_cumprod, dtype=np.float64)
    if kind == "euler":
        sig = np.asarray(t.sigmas, dtype=np.float64)
        out, trace = euler_loop(t.timesteps, sig, x, lambda x, i, tt: (x - x0) / sig[i])
    else:
        def eps(x, i, tt):
            at = ac[int(tt)]
            return (x - at ** 0.5 * x0) / (1 - at) ** 0.5
        if kind == "pndm":
            out, trace = plms_loop(t.timesteps, ac, n, x, eps)
        else:
            out, trace = dpm_loop(t.timesteps, ac, order, x, eps)
    return x0, noise, out, trace, t.source_levels()


def _residual(x0, out):
    return ((out - x0).pow(2).mean().sqrt() / x0.pow(2).mean().sqrt()).item()


@pytest.mark.parametrize("kind", list(KINDS))
@pytest.mark.parametrize("n", (10, 20, 50))
def test_point_mass_identity_returns_the_source(kind, n):
    """With eps = (x - a_t x0) / b_t (Euler: (x - x0) / sigma) every solver here is exact, so a loop started from start_level() walks
    a_i x0 + b_i noise through source_levels() and ends on x0 - up to the level of the schedule's last landing point, which for PNDM
    and DPM-Solver++ is alphas_cumprod[0] = 0.99915, not 1.  The residual is rms(x_final - x0) / rms(x0) (an rms, so that fp64
    rounding noise compares stably between two runs); the truncated runs must stay within 2x the full schedule's.

    Measured (fp64, seed 7; n = 10 / 20 / 50):
      Euler  full 1.117e-18 / 1.127e-18 / 1.036e-18   truncated (0.3, 0.5, 0.8) 1.098e-18 .. 1.150e-18, at most 1.11x the full one
             (almost every element returns to x0 exactly; what is left is a few last-place roundings)
      PNDM   full 2.692e-2 for every n                truncated 2.692e-2 for every (n, strength): 1.00x
      DPM-2  full 2.692e-2 for every n                truncated 2.692e-2 for every (n, strength): 1.00x
             (2.692e-2 = the landing level alphas_cumprod[0] of both solvers on this x0 / noise pair)
    """
    x0, _, out, _, _ = _point_mass_run(kind, n, 1.0)
    full = _residual(x0, out)
    print(f"{kind} n={n}: full-schedule residual {full:.3e}")
    for strength in (0.3, 0.5, 0.8):
        x0, noise, out, trace, levels = _point_mass_run(kind, n, strength)
        r = _residual(x0, out)
        print(f"{kind} n={n} strength={strength}: residual {r:.3e}")
        assert r <= 2 * full, (kind, n, strength, r, full)
        # the walk itself: after iteration i the state is the source at source_levels()[i] (the last one is the residual above)
        assert len(trace) == len(levels)
        for x, (a, b) in zip(trace[:-1], levels[:-1]):
            assert (x - (a * x0 + b * noise)).abs().max().item() <= 1e-9 * (1 + b)


@pytest.mark.parametrize("kind", list(KINDS))
def test_point_mass_identity_notices_a_wrong_start_level(kind):
    """Negative control: started one schedule position too high, the walk leaves the source levels."""
    n, strength = 20, 0.5
    wrong = KINDS[kind]().set_timesteps(n, 0.55).start_level()
    assert wrong != KINDS[kind]().set_timesteps(n, strength).start_level()
    x0, noise, out, trace, levels = _point_mass_run(kind, n, strength, start=wrong)
    a, b = levels[0]
    assert (trace[0] - (a * x0 + b * noise)).abs().max().item() > 1e-3
