"""The stochastic samplers without a GPU: the restated noise field (tests/sde_ref.py) against the Random123 known answers and its own
pinned moments; the restated Euler ancestral and SDE-DPM-Solver++ updates against identities that can be derived (data concentrated at
one point); the product tables against the restatement; the command line."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests.sde_ref import (RefEulerAncestral, RefSdeDpmSolver, field_fn, noise_field, noise_words, normals_from_words, philox4x32_10)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the noise field
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox_known_answers(counter, key, want):
    got = " ".join(f"{int(v):08x}" for v in philox4x32_10(counter, key))
    assert got == want


def test_counter_and_key_layout():
    """counter = (pixel, step, 0, 0), key = (low word, high word) of the seed."""
    seed = (7 << 32) + 5
    w = noise_words(seed, 49, 70)
    for pix in (0, 1, 69):
        assert [int(v) for v in w[pix]] == [int(v) for v in philox4x32_10((pix, 49, 0, 0), (5, 7))]
    assert not np.array_equal(noise_words(5, 49, 70), w)                 # the high word is part of the key
    assert not np.array_equal(noise_words(seed, 48, 70), w)
    assert np.array_equal(noise_words(seed + (1 << 64), 49, 70), w)      # 64-bit seed


def test_field_pin():
    """Seed 1234, step 3, pixels 0 .. 16383 (65 536 values): the moments of the fp64 restatement."""
    z, rad = normals_from_words(noise_words(1234, 3, 16384))
    z = z.reshape(-1)
    mean, std, m4, amax = z.mean(), z.std(), (z ** 4).mean(), np.abs(z).max()
    print(f"mean {mean:.12f} std {std:.12f} fourth moment {m4:.12f} max |z| {amax:.12f}")
    assert abs(mean - -0.004230144558) <= 1e-9
    assert abs(std - 0.997966271977) <= 1e-9
    assert abs(m4 - 2.972044133285) <= 1e-9
    assert abs(amax - 4.147865299104) <= 1e-9
    f, _ = noise_field(1234, 3, 128, 128)                                # [4, h, w]: channel c of pixel y * w + x
    assert f.shape == (4, 128, 128) and np.array_equal(f.reshape(4, -1).T.reshape(-1), z)


# ------------------------------------------------------------------------------------------------ point-mass identities (fp64)
@pytest.mark.parametrize("order", [1, 2])
def test_sde_dpm_solver_point_mass_identity(order):
    """Data concentrated at x*: the exact prediction is eps = (x - alpha_t x*) / sigma_t, x0 = x* at every step (so the second-order
    term vanishes), and a step maps x = alpha_s0 x* + sigma_s0 xi to alpha_p x* + sigma_p xi' with
    xi' = exp(-h) xi + sqrt(1 - exp(-2h)) z."""
    h_, w_ = 4, 5
    noise = field_fn(99, h_, w_)
    s = RefSdeDpmSolver(noise, order, dtype=torch.float64).set_timesteps(20)
    a, sg, lam = s.alpha_t, s.sigma_t, s.lambda_t
    g = torch.Generator().manual_seed(0)
    xstar = torch.randn(1, 4, h_, w_, generator=g, dtype=torch.float64)
    xi = torch.randn(1, 4, h_, w_, generator=g, dtype=torch.float64)
    ts = s.timesteps.tolist()
    x = a[ts[0]] * xstar + sg[ts[0]] * xi
    for i, t in enumerate(ts):
        p = 0 if i == len(ts) - 1 else ts[i + 1]
        hh = lam[p] - lam[t]
        # the two coefficient identities behind it
        assert abs(float(sg[p] / sg[t] * torch.exp(-hh) * a[t] + a[p] * (1 - torch.exp(-2 * hh)) - a[p])) <= 1e-12
        assert abs(float((sg[p] * torch.exp(-hh)) ** 2 + sg[p] ** 2 * (1 - torch.exp(-2 * hh)) - sg[p] ** 2)) <= 1e-12
        x = s.step((x - a[t] * xstar) / sg[t], t, x)["prev_sample"]
        xi = torch.exp(-hh) * xi + torch.sqrt(1 - torch.exp(-2 * hh)) * noise(i)
        err = (x - (a[p] * xstar + sg[p] * xi)).abs().max().item()
        assert err <= 1e-10, (order, i, err)


def test_euler_ancestral_point_mass_identity():
    """x = x* + sigma xi with the exact prediction eps = xi: sigma' xi' = sigma_down xi + sigma_up z, sigma_down^2 + sigma_up^2 =
    sigma'^2, and the last step (sigma' = 0, no noise) returns x*."""
    h_, w_ = 4, 5
    noise = field_fn(7, h_, w_)
    s = RefEulerAncestral(noise, dtype=torch.float64).set_timesteps(20)
    g = torch.Generator().manual_seed(1)
    xstar = torch.randn(1, 4, h_, w_, generator=g, dtype=torch.float64)
    xi = torch.randn(1, 4, h_, w_, generator=g, dtype=torch.float64)
    sig = s.sigmas.double()
    x = xstar + sig[0] * xi
    for i, t in enumerate(s.timesteps.tolist()):
        sg, sp, up, down = s.coefficients(i)
        assert abs(float(down ** 2 + up ** 2 - sp ** 2)) <= 1e-12 * max(1.0, float(sp ** 2))
        eps = (x - xstar) / sig[i]
        x = s.step(eps, t, x)["prev_sample"]
        want = xstar + down * eps + up * noise(i)                          # sigma' xi' = sigma_down xi + sigma_up z
        assert (x - want).abs().max().item() <= 1e-10 * max(1.0, float(sig[i])), i
    assert float(sig[-1]) == 0.0 and float(up) == 0.0
    assert (x - xstar).abs().max().item() <= 1e-12


def test_the_same_field_goes_to_every_row():
    noise = field_fn(3, 2, 3, torch.float32)
    for mk in (lambda: RefEulerAncestral(noise), lambda: RefSdeDpmSolver(noise)):
        both, alone = mk().set_timesteps(10), mk().set_timesteps(10)
        g = torch.Generator().manual_seed(2)
        x = torch.randn(1, 4, 2, 3, generator=g)
        xx, y = torch.cat([x, x]), x.clone()
        for t in both.timesteps.tolist()[:4]:
            e = torch.sin(y)
            xx = both.step(torch.cat([e, e]), t, xx)["prev_sample"]
            y = alone.step(e, t, y)["prev_sample"]
            assert torch.equal(xx[:1], y) and torch.equal(xx[1:], y)


# ------------------------------------------------------------------------------------------------ product tables
@pytest.mark.parametrize("strength", [1.0, 0.6])
@pytest.mark.parametrize("n", [10, 20, 50])
def test_product_tables_equal_the_restatement_bitwise(n, strength):
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables, EulerTables
    e = EulerAncestralTables().set_timesteps(n, strength)
    r = RefEulerAncestral(None, strength=strength).set_timesteps(n)
    assert e.kind == 4 and isinstance(e, EulerTables) and not hasattr(e, "solver_order")
    assert e.timesteps.dtype == np.float32 and np.array_equal(e.timesteps, r.timesteps.numpy())
    assert e.sigmas.dtype == np.float32 and np.array_equal(e.sigmas, r.sigmas.numpy()) and e.table() == r.sigmas.tolist()
    assert e.start_level() == r.start_level() and e.source_levels() == r.source_levels()
    assert e.source_levels()[-1] == (1, 0) and len(e.source_levels()) == len(e.timesteps)
    parent = EulerTables().set_timesteps(n, strength)
    assert np.array_equal(parent.sigmas, e.sigmas) and parent.source_levels() == e.source_levels()
    for order, kind in ((1, 5), (2, 6)):
        d = DPMSolverTables(solver_order=order, algorithm="sde-dpmsolver++").set_timesteps(n, strength)
        r = RefSdeDpmSolver(None, order, strength=strength).set_timesteps(n)
        assert d.kind == kind and d.solver_order == order and d.init_noise_sigma == 1
        assert d.timesteps.dtype == np.int64 and d.timesteps.tolist() == r.timesteps.tolist()
        assert np.array_equal(d.alphas_cumprod, r.alphas_cumprod.numpy()) and d.table() == r.alphas_cumprod.tolist()
        assert d.start_level() == r.start_level() and d.source_levels() == r.source_levels()
        assert d.source_levels()[-1] == (1, 0) and len(d.source_levels()) == len(d.timesteps)
        parent = DPMSolverTables(solver_order=order).set_timesteps(n, strength)
        assert parent.timesteps.tolist() == d.timesteps.tolist() and parent.source_levels() == d.source_levels()


def test_algorithm_keyword_defaults_and_errors():
    from rich_text_to_image_amd.schedulers import DPMSolverTables
    assert DPMSolverTables().kind == 3 and DPMSolverTables().algorithm == "dpmsolver++" and DPMSolverTables(solver_order=1).kind == 2
    assert DPMSolverTables(algorithm="sde-dpmsolver++").kind == 6
    with pytest.raises(ValueError):
        DPMSolverTables(algorithm="dpmsolver")


# ------------------------------------------------------------------------------------------------ command line
def _parse(argv):
    from rich_text_to_image_amd import sample
    return sample, sample.build_parser().parse_args(argv + ["--rich_text_json", "{}"])


def test_sample_flags_reach_the_pipeline_scheduler():
    import types
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables
    sample, a = _parse(["--scheduler", "sde-dpmsolver++", "--solver_order", "1"])
    m = sample.apply_scheduler(types.SimpleNamespace(scheduler="pipeline default"), a)
    assert isinstance(m.scheduler, DPMSolverTables) and m.scheduler.kind == 5 and m.scheduler.solver_order == 1
    sample, a = _parse(["--scheduler", "sde-dpmsolver++"])
    assert sample.make_scheduler(a).kind == 6
    sample, a = _parse(["--scheduler", "euler-ancestral", "--model", "SDXL"])
    m = sample.apply_scheduler(types.SimpleNamespace(scheduler="pipeline default"), a)
    assert isinstance(m.scheduler, EulerAncestralTables) and m.scheduler.kind == 4
    sample, a = _parse(["--scheduler", "euler-ancestral", "--model", "AnimeXL"])
    assert sample.make_scheduler(a).kind == 4
    sample, a = _parse(["--scheduler", "euler-ancestral", "--model", "SDXL", "--solver_order", "2"])
    with pytest.raises(SystemExit):
        sample.make_scheduler(a)


def test_euler_ancestral_is_refused_for_sd_by_name():
    sample, a = _parse(["--scheduler", "euler-ancestral", "--model", "SD"])
    with pytest.raises(SystemExit) as err:
        sample.make_scheduler(a)
    assert "euler-ancestral" in str(err.value) and "SD" in str(err.value)
    with pytest.raises(SystemExit) as err:                   # before any rank starts: main() ends before the launch
        sample.main(["--dry_launch", "--gpus", "2", "--model", "SD", "--scheduler", "euler-ancestral", "--rich_text_json", '{"ops": [{"insert": "a\\n"}]}'])
    assert "euler-ancestral" in str(err.value)


def test_requests_lines_may_name_a_scheduler(tmp_path):
    sample, a = _parse(["--model", "SDXL", "--scheduler", "dpmsolver++"])
    js = {"ops": [{"insert": "a\n"}]}
    f = tmp_path / "r.jsonl"
    f.write_text("\n".join(json.dumps(r) for r in ({"rich_text_json": js, "seed": 1, "scheduler": "euler-ancestral"},
                                                   {"rich_text_json": js, "seed": 2},
                                                   {"rich_text_json": js, "seed": 3, "scheduler": "sde-dpmsolver++"})))
    a.requests, a.rich_text_json = str(f), None
    reqs = sample.build_requests(a)
    assert [r["scheduler"] for r in reqs] == ["euler-ancestral", None, "sde-dpmsolver++"]
    # what main() does per request: the line's scheduler for that request only, the flag's for the others
    import types
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables
    a.solver_order = 1
    model = sample.apply_scheduler(types.SimpleNamespace(scheduler="pipeline default"), a)
    flag = model.scheduler
    assert isinstance(flag, DPMSolverTables) and flag.kind == 2
    seen = [sample.apply_request_scheduler(model, flag, r, a).scheduler for r in reqs]
    assert isinstance(seen[0], EulerAncestralTables) and seen[0].kind == 4            # --solver_order does not apply to it
    assert seen[1] is flag
    assert isinstance(seen[2], DPMSolverTables) and seen[2].kind == 5 and seen[2].solver_order == 1
    assert sample.apply_request_scheduler(model, flag, reqs[1], a).scheduler is flag   # back on the flag's after a line's own
    a.solver_order = None
    a.model = "SD"
    with pytest.raises(SystemExit):
        sample.build_requests(a)
    for bad in ("heun", "default"):
        f.write_text(json.dumps({"rich_text_json": js, "scheduler": bad}))
        with pytest.raises(SystemExit) as err:
            sample.build_requests(a)
        assert bad in str(err.value)


def _json_lines(text):
    return [json.loads(l) for l in text.splitlines() if l.startswith("{")]


@pytest.mark.parametrize("flags,want", [
    (["--scheduler", "euler-ancestral"], {"class": "EulerAncestralTables", "kind": 4, "solver_order": None}),
    (["--scheduler", "sde-dpmsolver++", "--solver_order", "1"], {"class": "DPMSolverTables", "kind": 5, "solver_order": 1}),
], ids=["euler_ancestral", "sde_dpm"])
def test_sample_scheduler_flags_hold_on_every_rank_dry_launch(tmp_path, flags, want):
    a = tmp_path / "a.json"
    a.write_text(json.dumps({"ops": [{"insert": "a "}, {"attributes": {"font": "slabo"}, "insert": "night sky"}, {"insert": "\n"}]}))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT", "MASTER_ADDR")}
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    base = [sys.executable, "-m", "rich_text_to_image_amd.sample", "--model", "SDXL", "--gpus", "2", "--dry_launch", "--split_image",
            "--rich_text_json", str(a), "--seeds", "0", "1"]
    out = subprocess.run(base + flags, env=env, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert out.returncode == 0, out.stderr[-2000:]
    lines = sorted(_json_lines(out.stdout), key=lambda d: d["rank"])
    assert [l["rank"] for l in lines] == [0, 1]
    for l in lines:
        assert l["scheduler"] == want, l
