"""CPU: the fp64 step restatement of tests/step_ref.py, which tests/test_step_epilogue_gpu.py holds the PLMS / Euler epilogue to.

It is pinned to the oracle loops (themselves pinned to the unmodified reference loops by tests/test_oracle.py) driven by a stub UNet, to
the product's scheduler tables, and to the analytic probability-flow ODE; and every named mutation of it moves a one-step output of the
GPU matrix by far more than the GPU bar."""
import numpy as np
import pytest
import torch

from oracle import region_loop
from oracle.schedulers import OracleEuler, OraclePNDM
from tests import step_ref as S


class StubUNet:
    """Returns the pre-drawn prediction of (step, stream) in the order the oracle loops call the UNet: uncond, base, [uncond_ref,
    text_ref,] regions (rich) or one batch-2 call [uncond; text] (plain)."""

    def __init__(self, steps, order):
        self.steps, self.order, self.k = steps, order, 0

    def forward(self, x, t, emb, added=None, ctl=None, store=None):
        i, j = divmod(self.k, len(self.order))
        self.k += 1
        role = self.order[j]
        return torch.cat([self.steps[i][r] for r in role]) if isinstance(role, tuple) else self.steps[i][role]


def _oracle_case(kind, mode, R, n, isa=0.0, ibg=0.0, hw=(8, 8)):
    return S._c(f"pin_{kind}_{mode}_{R}_{n}_{isa}_{ibg}", kind, mode, R, n, lat=hw, isa=isa, ibg=ibg)


PIN = ([_oracle_case("plms", "rich", R, n, isa, ibg) for n in (1, 2, 3, 4, 5, 10, 50) for R, isa, ibg in ((2, 0.5, 0.3), (1, 0.0, 0.5), (4, 0.3, 0.0))]
       + [_oracle_case("euler", "rich", R, n, 0.5, 0.3) for n in (1, 2, 3, 10) for R in (1, 4)]
       + [_oracle_case("euler", "rich", R, n, 0.0, 0.5) for n in (1, 2, 3, 4, 5, 10) for R in (2,)]
       + [_oracle_case("euler", "rich", 2, 50, 0.0, ibg) for ibg in (0.14, 0.3, 0.58)]
       + [_oracle_case(k, "plain", 0, n) for k in ("plms", "euler") for n in (1, 2, 3, 4, 5, 10, 50)])


@pytest.mark.parametrize("case", PIN, ids=[c["name"] for c in PIN])
def test_restatement_matches_the_oracle_loops(case):
    """The oracle schedulers and loops run in fp64 on the same predictions (fp32 tables, as in the product); every step within 1e-5."""
    x, M, steps = S.case_inputs(case)
    x, M = x.double(), [m.double() for m in M]
    steps = [{k: v.double() for k, v in s.items()} for s in steps]
    n, R, g = case["n"], case["R"], case["g"]
    sched = OracleEuler() if case["xl"] else OraclePNDM()
    trace = []
    if case["mode"] == "plain":
        lat = x
        unet = StubUNet(steps, [("u", "b")])
        sched.set_timesteps(n)
        for t in sched.timesteps:          # plain_loop without the trace argument, restated call for call
            eps = unet.forward(torch.cat([lat] * 2), t, None)
            eu, et = eps.chunk(2)
            lat = sched.step(eu + g * (et - eu), t, lat)["prev_sample"]
            trace.append(lat)
        assert torch.equal(lat, region_loop.plain_loop(StubUNet(steps, [("u", "b")]), OracleEuler() if case["xl"] else OraclePNDM(),
                                                       None, x, n, g, xl=case["xl"]))
    else:
        use_ref = case["isa"] > 0 or case["ibg"] > 0
        order = ["u", "b"] + (["ur", "tr"] if use_ref else []) + [f"r{k}" for k in range(R - 1)]
        unet = StubUNet(steps, order)
        if case["xl"]:
            region_loop.rich_loop_xl(unet, sched, torch.zeros(R + 1, 1, 1), torch.zeros(R + 1, 1), torch.zeros(1, 6), M, x, n, g, None,
                                     case["isa"], case["ibg"], trace=trace)
        else:
            region_loop.rich_loop_sd(unet, sched, torch.zeros(R + 1, 1, 1), M, x, n, g, None, case["isa"], case["ibg"], trace=trace)
    mine = S.run_restated(case)
    assert len(trace) == len(mine) == len(steps)
    worst = 0.0
    for i, (a, (b, _)) in enumerate(zip(trace, mine)):
        err = (a - b).abs().max().item() / b.abs().max().item()
        worst = max(worst, err)
        assert err <= 1e-5, (i, err)
    print(f"{case['name']}: worst relative step difference {worst:.2e}")


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 10, 50, 200])
def test_tables_are_the_products(n):
    from rich_text_to_image_amd.schedulers import EulerTables, PNDMTables
    p = PNDMTables().set_timesteps(n)
    assert p.timesteps.tolist() == S.plms_timesteps(n) and p.table() == S.PLMS(n).table()
    e = EulerTables().set_timesteps(n)
    ts, sig = S.euler_schedule(n)
    assert np.array_equal(e.timesteps, ts) and np.array_equal(e.sigmas, sig) and e.table() == S.Euler(n).table()


def test_the_xl_rule_at_rounding_edges():
    """int(ibg * n) and i < ibg * n on Python floats: 0.14 * 50 steps the pair at step 7 and blends there, 0.3 * 50 blends at 15 from an
    unstepped pair, 0.58 * 50 blends at 28 with the pair still stepped."""
    ts = S.Euler(50).timesteps
    p = lambda i, ibg: S.plan(i, ts, 2, 0.0, ibg, True)
    assert p(7, 0.14)["blend"] and p(7, 0.14)["step_ref"] and not p(8, 0.14)["step_ref"]
    assert p(15, 0.3)["blend"] and not p(15, 0.3)["step_ref"] and p(14, 0.3)["step_ref"]
    assert p(28, 0.58)["blend"] and p(28, 0.58)["step_ref"] and not p(29, 0.58)["step_ref"]
    assert S.plan(15, ts, 2, 0.0, 0.3, True, mutations=("xl_le",))["step_ref"]


@pytest.mark.parametrize("name", [c["name"] for c in S.CASES if c["elide"]])
def test_elision_leaves_lat_unchanged(name):
    """The pair stops part-way (the elided cases are chosen so) and lat is bit-identical with the unelided restatement."""
    c = S.CASE[name]
    stepped = [S.plan(i, S.make_sched(c["kind"], c["n"]).timesteps, c["R"], c["isa"], c["ibg"], c["xl"], True)["run_ref"]
               for i in range(len(S.make_sched(c["kind"], c["n"]).timesteps))]
    assert stepped[0] and not stepped[-1]
    for (a, _), (b, _) in zip(S.run_restated(c, elide=True), S.run_restated(c, elide=False)):
        assert torch.equal(a, b)


@pytest.mark.parametrize("name", [c["name"] for c in S.CASES if c["n"] <= 10])
def test_an_fp32_evaluation_stays_within_the_bar(name):
    """The restatement evaluated in fp32 from fp32 states (what any correct fp32 kernel does, up to operation order) stays within the
    one-step bar ULPS * u * magnitude of its fp64 evaluation: the bar is attainable."""
    c = S.CASE[name]
    x, M, steps = S.case_inputs(c)
    s32, s64 = S.make_sched(c["kind"], c["n"]), S.make_sched(c["kind"], c["n"])
    lat, lat_ref, worst = x, x.clone(), 0.0
    for i, ep in enumerate(steps):
        if c["mode"] == "plain":
            a = {"lat": S.plain_step(s32, i, ep["u"], ep["b"], lat, c["g"])}
            b = {"lat": S.plain_step(s64, i, ep["u"].double(), ep["b"].double(), lat.double(), c["g"])}
        else:
            args = (c["g"], c["isa"], c["ibg"], c["xl"], c["elide"])
            a = S.rich_step(s32, i, ep, M, lat, lat_ref, *args)
            b = S.rich_step(s64, i, {k: v.double() for k, v in ep.items()}, [m.double() for m in M], lat.double(), lat_ref.double(), *args)
        for k in b:
            if k in ("lat", "lat_ref", "noise_pred"):
                worst = max(worst, ((a[k][0].double() - b[k][0]).abs() / (S.ULPS * S.U32 * b[k][1])).max().item())
        lat = a["lat"][0]
        lat_ref = a["lat_ref"][0] if "lat_ref" in a else lat_ref
    print(f"{name}: fp32 evaluation worst error / bar {worst:.3f}")
    assert worst < 0.5, worst


def test_mutations_are_caught_by_the_gpu_bar():
    """Every mutation moves some one-step output of the GPU matrix's inputs by >= 100x the one-step bar."""
    margins = {}
    for m in S.MUTATIONS:
        margins[m] = max(S.one_step_margins(c, (m,)) for c in S.CASES)
        print(f"mutation {m}: worst one-step change {margins[m]:.3g} x the bar")
    assert all(v >= 100 for v in margins.values()), margins
    assert S.one_step_margins(S.CASES[0], ()) == 0.0


def _ode(kind, n, c=2.0, hw=32):
    """Data ~ N(0, c^2), exact noise predictions: the restated sampler's end point against the exact probability-flow solution."""
    s = S.make_sched(kind, n)
    x = torch.linspace(-3, 3, 4 * hw * hw, dtype=torch.float64).reshape(1, 4, hw, hw)
    if kind == "euler":
        sig = s.sigmas
        x = x * (sig[0] ** 2 + 1) ** 0.5
        exact = x * c / (c * c + sig[0] ** 2) ** 0.5
        for i in range(n):
            e = sig[i] * x / (c * c + sig[i] ** 2)
            x = S.plain_step(s, i, e, e, x, 1.0)[0]
    else:
        ac = S.alphas_cumprod().double()
        var = lambda t: (ac[t] * c * c + (1 - ac[t])).item()
        exact = x * (var(0) / var(s.timesteps[0])) ** 0.5
        for i, t in enumerate(s.timesteps):
            e = (1 - ac[t].item()) ** 0.5 * x / var(t)
            x = S.plain_step(s, i, e, e, x, 1.0)[0]
    return (x - exact).abs().max().item()


def test_analytic_ode_errors():
    """Euler converges at first order; PLMS does not converge cleanly (its last step lands on alphas_cumprod[0] with unequal spacing)."""
    eul = {n: _ode("euler", n) for n in (10, 20, 50, 100, 200)}
    for n, want in {10: 0.555, 20: 0.297, 50: 0.124, 100: 0.0635, 200: 0.0326}.items():
        assert abs(eul[n] - want) <= 0.01 * want, (n, eul[n])
    assert all(1.8 <= eul[a] / eul[b] <= 2.2 for a, b in ((10, 20), (50, 100), (100, 200))), eul
    for n, want in {10: 8.99e-3, 50: 3.58e-4, 200: 2.15e-4}.items():
        assert abs(_ode("plms", n) - want) <= 0.01 * want, n
