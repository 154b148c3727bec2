"""The step epilogue alone, one solver family after the other - Euler, DPM-Solver++(2M), the two stochastic samplers (Euler ancestral,
SDE-DPM-Solver++(2M): one Philox call + two Box-Muller pairs per pixel) and, when named, PLMS - at SDXL's 128 x 128 latents: R = 4 regions
with the reference pair stepped (F = 7 streams, inject_selfattn 0.5), seeded noise predictions in the eps buffer, no UNet.  Meant to run
under `rocprofv3 --kernel-trace --stats -- python tools/dpm_epilogue_profile.py [sampler ...]`: every instantiation of
step_epilogue_kernel<solver> (csrc/step.hip) has a row of its own in the kernel statistics.  Without arguments the four samplers an SDXL
pass can run; `plms` is run by name.  Also prints a HIP-event mean per launch."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(names, hw=128, R=4, steps=50, reps=4):
    from oracle.unet import TINY_SD_CONFIG
    from rich_text_to_image_amd.engine import Engine
    from rich_text_to_image_amd.launcher import eps_tensor
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables, EulerTables, PNDMTables
    dev = "cuda:0"
    e = Engine(TINY_SD_CONFIG, hw, hw, device=0, max_streams=8, max_prompts=8)
    e.arena_mark_bound()                                        # the UNet never runs here
    g = torch.Generator().manual_seed(0)
    e.set_prompts(torch.randn(R + 1, 77, TINY_SD_CONFIG["cross_attention_dim"], generator=g).to(dev))
    e.set_masks(torch.softmax(torch.randn(R, 1, hw, hw, generator=g), 0).repeat(1, 4, 1, 1).to(dev))
    lat0 = torch.randn(1, 4, hw, hw, generator=g).to(dev)
    e.set_latents(lat0)                                         # (sizes the eps buffer's streams)
    buf, per = eps_tensor(e)
    buf.view(torch.float32)[:(per // 4) * (R + 3)].copy_(torch.randn((per // 4) * (R + 3), generator=g).to(dev))
    samplers = {"euler": EulerTables, "dpmsolver++": DPMSolverTables, "euler-ancestral": EulerAncestralTables,
                "sde-dpmsolver++": lambda: DPMSolverTables(algorithm="sde-dpmsolver++"), "plms": PNDMTables}
    out = {}
    for rep in range(reps):
        for name in names:
            s = samplers[name]()
            s.set_timesteps(steps)
            e.set_schedule(s.kind, s.timesteps.tolist(), s.table(), steps)
            e.set_noise_seed(rep)
            e.set_latents(lat0)
            e.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for i in range(len(s.timesteps)):
                e.region_step_finish(i, 5.0, 0.5, 0.0, name != "plms")
            b.record(); e.synchronize(); torch.cuda.synchronize()
            out.setdefault(name, []).append(a.elapsed_time(b) * 1e3 / len(s.timesteps))
            assert torch.isfinite(e.read_latents(hw, hw)).all()
    for name, v in out.items():
        print(f"{name}: {min(v):.2f} us per epilogue launch (HIP events over {steps} back-to-back launches, best of {reps})")
    e.close()


if __name__ == "__main__":
    main(sys.argv[1:] or ["euler", "dpmsolver++", "euler-ancestral", "sde-dpmsolver++"])
