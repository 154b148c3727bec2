"""The PLMS and Euler step epilogues (csrc/step.hip step_epilogue_kernel<STEP_PLMS / STEP_EULER> + csrc/step_driver.inl region_plan /
finish_step / pndm_coeffs / plain_finish) in isolation, every step, against the fp64 restatement of tests/step_ref.py.

A tiny engine whose arena is only marked bound (the UNet never runs); seeded noise predictions go straight into the eps slots of the
step's streams, every other slot holds NaN, then region_step_finish / plain_step_finish.  Each step is checked twice: one step of the
restatement from the GPU's own previous latents and the same prediction history (bar: ULPS * u * the expression's magnitude), and the
accumulated trajectory (1e-5 * (i + 1) * max|x|)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle.unet import TINY_SD_CONFIG  # noqa: E402
from tests import step_ref as S  # noqa: E402

DEV = "cuda:0"
NAN = float("nan")


def _engine(case, n_prompts, max_streams=16, max_prompts=14):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(TINY_SD_CONFIG, case["eng"][0], case["eng"][1], device=0, max_streams=max_streams, max_prompts=max_prompts)
    e.arena_mark_bound()
    g = torch.Generator().manual_seed(9)
    e.set_prompts(torch.randn(n_prompts, 77, TINY_SD_CONFIG["cross_attention_dim"], generator=g).to(DEV))
    return e


def _set_schedule(e, case):
    s = S.make_sched(case["kind"], case["n"])
    e.set_schedule(s.kind, s.timesteps, s.table(), case["n"])


def _view(ptr, nfloat):
    from rich_text_to_image_amd.launcher import _DevicePointer
    return torch.as_tensor(_DevicePointer(ptr, nfloat * 4), device=DEV).view(torch.float32)


class Run:
    """One pass over a case's schedule on engine `e`; `check` compares every step with the restatement."""

    def __init__(self, e, case, inputs, elide=None, defer=None):
        self.e, self.c = e, case
        self.x, self.M, self.steps = inputs
        self.elide = case["elide"] if elide is None else elide
        self.defer = case["defer"] if defer is None else defer
        h, w = case["lat"]
        self.hw = h * w
        self.worst = dict(lat=0.0, lat_ref=0.0, noise_pred=0.0, trajectory=0.0)

    @property
    def eps(self):
        """The eps buffer at the latents' size (rt_eps_info needs rt_set_latents first)."""
        from rich_text_to_image_amd.launcher import eps_tensor
        buf, per = eps_tensor(self.e)
        assert per == self.hw * 16
        return buf.view(torch.float32)

    def put(self, s, x):
        self.eps[s * self.hw * 4:(s + 1) * self.hw * 4].copy_(x.reshape(4, self.hw).t().reshape(-1))

    def step(self, i, ep):
        c, e = self.c, self.e
        self.eps.fill_(NAN)
        if c["mode"] == "plain":
            self.put(0, ep["u"].to(DEV)); self.put(1, ep["b"].to(DEV))
            torch.cuda.synchronize()                           # the engine launches on a stream of its own
            e.plain_step_finish(i, c["g"])
            return None
        p = S.plan(i, self.sched_ts, c["R"], c["isa"], c["ibg"], c["xl"], self.elide)
        for s, role in enumerate(p["streams"]):
            if role in ("ur", "tr") and not p["step_ref"]:
                continue                                   # the pair's slots stay NaN on a step that does not step it
            self.put(s, ep[role].to(DEV))
        torch.cuda.synchronize()
        e.region_step_finish(i, c["g"], c["isa"], c["ibg"], c["xl"], elide=self.elide, defer_blend=self.defer)
        if self.defer:
            e.background_blend()
        return p

    def go(self, check=True, between=None, upto=None):
        c, e = self.c, self.e
        h, w = c["lat"]
        e.set_latents(self.x.to(DEV))
        one, traj = S.make_sched(c["kind"], c["n"]), S.make_sched(c["kind"], c["n"])
        self.sched_ts = one.timesteps
        M64 = [m.double() for m in self.M]
        prev, prev_ref = (t.cpu().double() for t in e.read_latents(h, w, with_ref=True))
        t_lat, t_ref = prev.clone(), prev_ref.clone()
        lats = []
        for i, ep in enumerate(self.steps[:upto]):
            p = self.step(i, ep)
            got, got_ref = (t.cpu() for t in e.read_latents(h, w, with_ref=True))
            lats.append(got)
            if check:
                ep64 = {k: v.double() for k, v in ep.items()}
                if p is None:
                    r = {"lat": S.plain_step(one, i, ep64["u"], ep64["b"], prev, c["g"])}
                    t_lat = S.plain_step(traj, i, ep64["u"], ep64["b"], t_lat, c["g"])[0]
                    outs = {"lat": got}
                else:
                    r = S.rich_step(one, i, ep64, M64, prev, prev_ref, c["g"], c["isa"], c["ibg"], c["xl"], self.elide)
                    rt = S.rich_step(traj, i, ep64, M64, t_lat, t_ref, c["g"], c["isa"], c["ibg"], c["xl"], self.elide)
                    t_lat, t_ref = rt["lat"][0], rt["lat_ref"][0]
                    npred = _view(e.state_ptrs()[1], 4 * self.hw).clone().cpu().reshape(1, 4, h, w)
                    outs = {"lat": got, "lat_ref": got_ref, "noise_pred": npred}
                    if not p["step_ref"]:
                        assert torch.equal(got_ref.double(), prev_ref), (c["name"], i, "the unstepped reference latents moved")
                for k, g in outs.items():
                    assert torch.isfinite(g).all(), (c["name"], i, k, "a poisoned slot was read")
                    ratio = ((g.double() - r[k][0]).abs() / (S.ULPS * S.U32 * r[k][1])).max().item()
                    self.worst[k] = max(self.worst[k], ratio)
                    assert ratio <= 1.0, (c["name"], i, k, ratio)
                err = (got.double() - t_lat).abs().max().item() / (1e-5 * (i + 1) * t_lat.abs().max().item())
                self.worst["trajectory"] = max(self.worst["trajectory"], err)
                assert err <= 1.0, (c["name"], i, "trajectory", err)
                prev, prev_ref = got.double(), got_ref.double()
            if between is not None:
                between(i)
        return lats


@pytest.mark.parametrize("name", [c["name"] for c in S.CASES])
def test_epilogue_matches_the_restatement_every_step(name):
    c = S.CASE[name]
    inputs = S.case_inputs(c)
    e = _engine(c, 2 if c["mode"] == "plain" else c["R"] + 1)
    try:
        if c["mode"] != "plain":
            e.set_masks([m.to(DEV) for m in inputs[1]])
        _set_schedule(e, c)
        run = Run(e, c, inputs)
        first = run.go()
        print(f"{name}: worst error / bar  " + "  ".join(f"{k} {v:.3f}" for k, v in run.worst.items() if v or k == "lat"))
        # the PLMS / Euler state really resets: a second pass after set_latents reproduces the first bit for bit
        again = Run(e, c, inputs).go(check=False)
        assert all(torch.equal(a, b) for a, b in zip(first, again)), "second pass after set_latents"
        if c["mode"] == "plain":
            # ... and after set_schedule alone: dirty the state, put x_T back through the latents pointer, set_schedule, run again
            Run(e, c, inputs).go(check=False, upto=2)
            h, w = c["lat"]
            _view(e.state_ptrs()[0], 4 * h * w).copy_(inputs[0].reshape(-1).to(DEV))
            torch.cuda.synchronize()
            _set_schedule(e, c)
            r = Run(e, c, inputs)
            r.sched_ts = None
            lats = []
            for i, ep in enumerate(inputs[2]):
                r.step(i, ep)
                lats.append(e.read_latents(h, w).cpu())
            assert all(torch.equal(a, b) for a, b in zip(first, lats)), "second pass after set_schedule"
        if c["elide"]:
            # with stubbed predictions the elided pass and the full pass leave bit-identical latents at every step
            full = Run(e, c, inputs, elide=False).go(check=False)
            assert all(torch.equal(a, b) for a, b in zip(first, full)), "elide"
        if c["defer"]:
            # a deferred blend followed by background_blend() equals the fused blend bit for bit
            fused = Run(e, c, inputs, defer=False).go(check=False)
            assert all(torch.equal(a, b) for a, b in zip(first, fused)), "deferred blend"
    finally:
        e.close()


def _ode_run(kind, n, c=2.0, hw=32):
    """plain_step_finish, g = 1: every step reads the latents back and writes the exact noise prediction of data ~ N(0, c^2) into both
    slots; the restatement runs the same closed loop in fp64."""
    case = S._c(f"ode_{kind}_{n}", kind, "plain", 0, n, lat=(hw, hw))
    e = _engine(case, 2)
    try:
        _set_schedule(e, case)
        s = S.make_sched(kind, n)
        x = torch.linspace(-3, 3, 4 * hw * hw, dtype=torch.float64).reshape(1, 4, hw, hw)
        if kind == "euler":
            x = x * (s.sigmas[0] ** 2 + 1) ** 0.5
            eps_of = lambda i, y: s.sigmas[i] * y / (c * c + s.sigmas[i] ** 2)
            exact = x * c / (c * c + s.sigmas[0] ** 2) ** 0.5
        else:
            ac = S.alphas_cumprod().double()
            var = lambda t: (ac[t] * c * c + (1 - ac[t])).item()
            eps_of = lambda i, y: (1 - ac[s.timesteps[i]].item()) ** 0.5 * y / var(s.timesteps[i])
            exact = x * (var(0) / var(s.timesteps[0])) ** 0.5
        e.set_latents(x.float().to(DEV))
        from rich_text_to_image_amd.launcher import eps_tensor
        buf, per = eps_tensor(e)
        f = buf.view(torch.float32)
        n_hw = hw * hw
        ref, x_ref = S.make_sched(kind, n), x.float().double()
        for i in range(len(s.timesteps)):
            y = e.read_latents(hw, hw).cpu().double()
            eps = eps_of(i, y).float().reshape(4, n_hw).t().reshape(-1).to(DEV)
            f[:n_hw * 4].copy_(eps); f[n_hw * 4:2 * n_hw * 4].copy_(eps)
            torch.cuda.synchronize()
            e.plain_step_finish(i, 1.0)
            x_ref = S.plain_step(ref, i, eps_of(i, x_ref), eps_of(i, x_ref), x_ref, 1.0)[0]
        got = e.read_latents(hw, hw).cpu().double()
    finally:
        e.close()
    return (got - x_ref).abs().max().item() / x_ref.abs().max().item(), (got - exact).abs().max().item()


def test_analytic_ode_through_plain_step_finish():
    """Euler shows first order; PLMS (whose last step lands on alphas_cumprod[0] with unequal spacing) only agrees with the restatement."""
    eul = {}
    for n in (10, 20, 50, 100, 200):
        rel, eul[n] = _ode_run("euler", n)
        print(f"euler n={n}: engine vs restatement {rel:.2e}, error {eul[n]:.4g}")
        assert rel <= 1e-5, (n, rel)
    assert all(1.8 <= eul[a] / eul[b] <= 2.2 for a, b in ((10, 20), (50, 100), (100, 200))), eul
    for n in (10, 50, 200):
        rel, err = _ode_run("plms", n)
        print(f"plms n={n}: engine vs restatement {rel:.2e}, error {err:.4g}")
        assert rel <= 1e-5, (n, rel)


@pytest.mark.parametrize("kind", ["plms", "euler"])
def test_error_paths_leave_the_engine_usable(kind):
    """Mid-run, a step index >= n, xl that does not match the scheduler, and R + 3 > max_streams raise RtError; the run then goes on and
    every later step still matches the restatement."""
    from rich_text_to_image_amd.engine import RtError
    c = S._c(f"errors_{kind}", kind, "rich", 6, 5, isa=0.0, ibg=0.0)       # 6 regions, no reference pair: 7 of 8 streams
    inputs = S.case_inputs(c)
    e = _engine(c, 7, max_streams=8, max_prompts=8)
    try:
        e.set_masks([m.to(DEV) for m in inputs[1]])
        _set_schedule(e, c)
        n = len(S.make_sched(kind, c["n"]).timesteps)
        raised = []

        def between(i):
            if i != 1:
                return
            for bad in (lambda: e.region_step_finish(n, c["g"], 0.0, 0.0, c["xl"]),
                        lambda: e.region_step_finish(-1, c["g"], 0.0, 0.0, c["xl"]),
                        lambda: e.region_step_finish(2, c["g"], 0.0, 0.0, not c["xl"]),
                        lambda: e.region_step_finish(2, c["g"], 0.5, 0.3, c["xl"]),        # + the reference pair: 9 streams
                        lambda: e.plain_step_finish(n, c["g"])):
                with pytest.raises(RtError):
                    bad()
                raised.append(1)

        Run(e, c, inputs).go(between=between)
        assert len(raised) == 5
    finally:
        e.close()
