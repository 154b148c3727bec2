"""What the guided-prediction pre-pass (csrc/guided.hip: two launches in front of the step epilogue) costs, at SDXL's 128 x 128 latents:
R = 4 regions with the reference pair stepped (F = 7 streams, inject_selfattn 0.5), seeded model outputs in the eps buffer, no UNet - the
set-up of tools/dpm_epilogue_profile.py.  For every sampler family the bare epilogue (prediction epsilon, rescale 0: today's launches)
against the epilogue behind the pre-pass with (epsilon, 0.7), (v, 0) and (v, 0.7): HIP-event mean per step over back-to-back steps,
best of `reps`."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main(hw=128, R=4, steps=50, reps=4):
    from oracle.unet import TINY_SD_CONFIG
    from rich_text_to_image_amd.engine import Engine
    from rich_text_to_image_amd.launcher import eps_tensor
    from rich_text_to_image_amd.schedulers import DPMSolverTables, EulerAncestralTables, EulerTables
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
    settings = (("bare epilogue", 0, 0.0), ("epsilon, rescale 0.7", 0, 0.7), ("v, rescale 0", 1, 0.0), ("v, rescale 0.7", 1, 0.7))
    out = {}
    for rep in range(reps):
        for name, s in (("euler", EulerTables()), ("dpmsolver++", DPMSolverTables()), ("euler-ancestral", EulerAncestralTables()),
                        ("sde-dpmsolver++", DPMSolverTables(algorithm="sde-dpmsolver++"))):
            s.set_timesteps(steps)
            for label, ptype, phi in settings:
                e.set_schedule(s.kind, s.timesteps.tolist(), s.table(), steps)
                e.set_noise_seed(rep)
                e.set_prediction(ptype, phi)
                e.set_latents(lat0)
                e.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for i in range(len(s.timesteps)):
                    e.region_step_finish(i, 5.0, 0.5, 0.0, True)
                b.record(); e.synchronize(); torch.cuda.synchronize()
                out.setdefault((name, label), []).append(a.elapsed_time(b) * 1e3 / len(s.timesteps))
    for (name, label), v in out.items():
        bare = min(out[(name, "bare epilogue")])
        extra = "" if label == "bare epilogue" else f"  (+{min(v) - bare:.2f} us for the two pre-pass launches)"
        print(f"{name}, {label}: {min(v):.2f} us per step finish{extra}")
    print(f"HIP events over {steps} back-to-back step finishes at {hw} x {hw}, {R + 3} streams, best of {reps}")
    e.close()


if __name__ == "__main__":
    main()
