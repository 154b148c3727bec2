"""One SHA-256 per case over the bits the step epilogue leaves, for comparing two builds of the library line for line.

Walks the case tables of the four epilogue GPU tests - tests/step_ref.py (PLMS, Euler), the (mode, order) grid of
tests/test_dpm_solver_gpu.py and the (mode, kind) grid of tests/test_stochastic_gpu.py on the schedules of tests/dpm_solver_ref.py and
tests/sde_ref.py, and tests/guided_ref.py (v-prediction, guidance rescale, all five solver families) - at their shapes, feeding their
seeded predictions the way tests/test_step_epilogue_gpu.py does: a tiny engine whose arena is only marked bound, the predictions written
straight into the eps slots of the step's streams, NaN everywhere else.  Only Engine.region_step_finish / plain_step_finish /
background_blend run.  The digest of a case covers, for every step, the bytes of lat and lat_ref and, for a rich step, noise_pred
(the plain step writes none).

    python tools/step_epilogue_digest.py > digests.txt
"""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

DEV = "cuda:0"
SEED = 41


def _grid_cases():
    """The (mode, order) grid of test_dpm_solver_gpu.py and the (mode, kind) grid of test_stochastic_gpu.py as case dicts with
    step_ref's keys; kind_no is the engine's schedule kind, read off the package's scheduler objects."""
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables
    kinds = {"dpm1": DPMSolverTables(solver_order=1).kind, "dpm2": DPMSolverTables(solver_order=2).kind,
             "sde1": DPMSolverTables(solver_order=1, algorithm="sde-dpmsolver++").kind,
             "sde2": DPMSolverTables(solver_order=2, algorithm="sde-dpmsolver++").kind, "euler_a": EulerAncestralTables.kind}

    def case(name, mode, n, lat=(32, 32), eng=(32, 32)):
        rich = mode != "plain"
        return dict(name=f"{name}_{mode}_" + (f"n{n}" if lat == (32, 32) else f"{lat[0]}x{lat[1]}"), kind=name, kind_no=kinds[name],
                    sigma_space=name == "euler_a", mode="rich" if rich else "plain", R=3 if rich else 0, n=n, lat=lat, eng=eng,
                    isa=0.5 if mode == "sd" else 0.0, ibg=0.3, elide=False, defer=False, xl=mode == "xl", g=7.5)

    out = [case(name, mode, n) for name in kinds for mode in ("sd", "xl", "plain") if not (name == "euler_a" and mode == "sd")
           for n in (20, 8)]                            # 8 < 15: the lower-order final step
    return out + [case("sde2", "sd", 20, lat=(12, 8)), case("euler_a", "xl", 20, lat=(12, 8))]


def _grid_schedule(c):
    from tests.dpm_solver_ref import dpm_timesteps, scaled_linear_alphas_cumprod
    from tests.sde_ref import RefEulerAncestral
    if c["sigma_space"]:
        ref = RefEulerAncestral(None).set_timesteps(c["n"])
        return ref.timesteps.tolist(), ref.sigmas.tolist(), ref.init_noise_sigma
    return [float(t) for t in dpm_timesteps(c["n"])], scaled_linear_alphas_cumprod().tolist(), 1.0


def _grid_inputs(c, timesteps, sigma0):
    from tests import step_ref as S
    h, w = c["lat"]
    g = torch.Generator().manual_seed(4)
    R = max(c["R"], 1)
    m = torch.softmax(torch.randn(R, 1, h, w, generator=g) * 2, 0).repeat(1, 4, 1, 1)
    x = torch.randn(1, 4, h, w, generator=g) * sigma0
    steps = [{k: torch.randn(1, 4, h, w, generator=g) for k in S.roles(R)} for _ in timesteps]
    return x, [m[r:r + 1] for r in range(R)], steps


def digest(c, kind_no, timesteps, table, inputs, vpred=False, phi=0.0):
    from oracle.unet import TINY_SD_CONFIG
    from rich_text_to_image_amd.engine import Engine
    from rich_text_to_image_amd.launcher import _DevicePointer, eps_tensor
    from tests import step_ref as S
    x, M, steps = inputs
    h, w = c["lat"]
    hw = h * w
    rich = c["mode"] != "plain"
    e = Engine(TINY_SD_CONFIG, c["eng"][0], c["eng"][1], device=0, max_streams=16, max_prompts=14)
    try:
        e.arena_mark_bound()
        g = torch.Generator().manual_seed(9)
        e.set_prompts(torch.randn(c["R"] + 1 if rich else 2, 77, TINY_SD_CONFIG["cross_attention_dim"], generator=g).to(DEV))
        if rich:
            e.set_masks([m.to(DEV) for m in M])
        e.set_schedule(kind_no, timesteps, table, c["n"])
        e.set_noise_seed(SEED)
        e.set_prediction(int(vpred), phi)
        e.set_latents(x.to(DEV))
        buf, per = eps_tensor(e)
        assert per == hw * 16
        eps = buf.view(torch.float32)
        npred = torch.as_tensor(_DevicePointer(e.state_ptrs()[1], 4 * hw * 4), device=DEV).view(torch.float32)
        sha = hashlib.sha256()

        def put(s, t):
            eps[s * hw * 4:(s + 1) * hw * 4].copy_(t.reshape(4, hw).t().reshape(-1).to(DEV))

        for i, ep in enumerate(steps):
            eps.fill_(float("nan"))
            if not rich:
                put(0, ep["u"]); put(1, ep["b"])
                torch.cuda.synchronize()                       # the engine launches on a stream of its own
                e.plain_step_finish(i, c["g"])
            else:
                p = S.plan(i, timesteps, c["R"], c["isa"], c["ibg"], c["xl"], c["elide"])
                for s, role in enumerate(p["streams"]):
                    if role in ("ur", "tr") and not p["step_ref"]:
                        continue                               # the pair's slots stay NaN on a step that does not step it
                    put(s, ep[role])
                torch.cuda.synchronize()
                e.region_step_finish(i, c["g"], c["isa"], c["ibg"], c["xl"], elide=c["elide"], defer_blend=c["defer"])
                if c["defer"]:
                    e.background_blend()
            lat, lat_ref = e.read_latents(h, w, with_ref=True)
            for t in (lat, lat_ref) + ((npred.clone(),) if rich else ()):
                assert torch.isfinite(t).all(), (c["name"], i, "a poisoned slot was read")
                sha.update(t.cpu().contiguous().numpy().tobytes())
        return sha.hexdigest()
    finally:
        e.close()


def main():
    from tests import guided_ref as G
    from tests import step_ref as S
    for c in S.CASES:
        s = S.make_sched(c["kind"], c["n"])
        print(f"step_ref/{c['name']} {digest(c, s.kind, s.timesteps, s.table(), S.case_inputs(c))}", flush=True)
    for c in _grid_cases():
        ts, table, sigma0 = _grid_schedule(c)
        print(f"grid/{c['name']} {digest(c, c['kind_no'], ts, table, _grid_inputs(c, ts, sigma0))}", flush=True)
    for c in G.CASES:
        s = G.make_sched(c["kind"], c["n"])
        print(f"guided_ref/{c['name']} {digest(c, G.KINDS[c['kind']], s.timesteps, s.table(), G.case_inputs(c), c['vpred'], c['phi'])}", flush=True)


if __name__ == "__main__":
    main()
