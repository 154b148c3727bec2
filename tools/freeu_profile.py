"""What FreeU (csrc/freeu.hip) costs at SDXL's 128 x 128 latents with the 7 streams of an injected rich-text step.

  kernels   the six concatenations of up blocks 0 and 1 - (C1, C2) = (1280, 1280), (1280, 1280), (1280, 640) on the 32 x 32 grid and
            (1280, 640), (640, 640), (640, 320) on the 64 x 64 grid - through rt_op_freeu on seeded fp16 tensors: HIP events over
            `launches` back-to-back calls, best of `reps`, for the skip filter alone, the backbone scaling alone and both.  Bytes: the
            skip read twice and written once, half of the hidden tensor read and written once; the rate they give stands beside a
            device-to-device copy of the same tensors timed the same way (a large float4 copy reaches 6.29 TB/s on this chip).
            Every shape runs the ONE form the kernel has: one launch per half, the workgroup of a (stream, 32-channel slab) walks its
            tokens twice (the second walk re-reads what the same thread just read).
  step      (--step) bench.py's workload - SDXL, R = 4, inject_selfattn 0.5, 50-step Euler, seeded weights and inputs - timed with
            FreeU on against off in alternated pairs on one engine: ms per step over `steps` steps with bench.py's stride over the schedule.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((32, 32, 1280, 1280), (32, 32, 1280, 1280), (32, 32, 1280, 640), (64, 64, 1280, 640), (64, 64, 640, 640), (64, 64, 640, 320))
SDXL_FREEU = (0.6, 0.4, 1.1, 1.2)          # diffusers' suggestion for SDXL (s1, s2, b1, b2)


def _timed(fn, launches, reps):
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / launches)
    return best


def kernels(B=7, launches=200, reps=5):
    import ctypes as C
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    total = 0.0
    for (H, W, C1, C2) in SHAPES:
        hid = torch.randn(B, H * W, C1, generator=g).half().to(dev)
        sk = (torch.randn(B, H * W, C2, generator=g) + torch.randn(C2, generator=g)).half().to(dev)
        hid2, sk2 = torch.empty_like(hid), torch.empty_like(sk)

        def op(h, s, b, sc):
            rc = lib.rt_op_freeu(C.c_void_p(h.data_ptr() if h is not None else 0), C1, C.c_void_p(s.data_ptr() if s is not None else 0), C2,
                                 B, H, W, C.c_float(b), C.c_float(sc), st)
            assert rc == 0, lib.rt_op_last_error().decode()
        # s, b close to 1 so that hundreds of in-place applications stay finite: the arithmetic and the traffic do not depend on the values
        for _ in range(3):
            op(hid, sk, 1.0009765625, 0.999)
        t_skip = _timed(lambda: op(None, sk, 1.0, 0.999), launches, reps)
        t_hid = _timed(lambda: op(hid, None, 1.0009765625, 1.0), launches, reps)
        t_both = _timed(lambda: op(hid, sk, 1.0009765625, 0.999), launches, reps)
        t_copy = _timed(lambda: (hid2.copy_(hid), sk2.copy_(sk)), launches, reps)
        by_skip, by_hid = 3.0 * sk.numel() * 2, 2.0 * (hid.numel() // 2) * 2
        by_copy = 2.0 * (sk.numel() + hid.numel()) * 2
        assert bool(torch.isfinite(sk.float()).all()) and bool(torch.isfinite(hid.float()).all())
        print(f"{H}x{W} C1 {C1} C2 {C2} B {B}: skip filter {t_skip:.1f} us ({by_skip / 1e6:.1f} MB, {by_skip / t_skip / 1e6:.2f} TB/s) | "
              f"backbone scaling {t_hid:.1f} us ({by_hid / 1e6:.1f} MB, {by_hid / t_hid / 1e6:.2f} TB/s) | both {t_both:.1f} us | "
              f"copy of both tensors (two launches) {t_copy:.1f} us ({by_copy / t_copy / 1e6:.2f} TB/s)")
        total += t_both
    print(f"all six concatenations, both halves: {total:.1f} us per forward of {B} streams "
          f"(HIP events over {launches} back-to-back launches, best of {reps}; one form for every shape: one launch per half, slab walked twice)")


def step(steps=20, pairs=3, warmup=3):
    import bench
    from rich_text_to_image_amd.engine import SDXL_CONFIG, Engine
    dev = "cuda:0"
    R, hw, nsched, gs, isa, ibg = 4, 128, 50, 5.0, 0.5, 0.0
    eng = Engine(SDXL_CONFIG, hw, hw, device=0, max_streams=8, max_prompts=8)
    g = torch.Generator(device=dev).manual_seed(0)
    for name, shape in eng.weight_table():
        if name.endswith(".weight") and len(shape) >= 2:
            t = (torch.rand(shape, generator=g, device=dev) * 2 - 1) / math.sqrt(math.prod(shape[1:]))
        elif name.endswith(".weight"):
            t = 1.0 + 0.1 * (torch.rand(shape, generator=g, device=dev) * 2 - 1)
        else:
            t = 0.05 * (torch.rand(shape, generator=g, device=dev) * 2 - 1)
        eng.bind_weight(name, t)
        eng.synchronize()
        del t
    inp = bench.synth_inputs(1000, R, hw, dev)
    ts, sig, init_sigma = bench.euler_tables(nsched)
    eng.set_prompts(inp["emb"], inp["pooled"], inp["tid"])
    eng.set_masks(inp["masks"])
    eng.set_fontsize(torch.tensor([5, 6]), torch.tensor([20.0, 20.0]))
    lat0 = (inp["lat"] * init_sigma).to(dev)

    def run(k):
        eng.set_schedule(0, ts, sig, nsched)
        eng.set_latents(lat0)
        eng.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(k):
            eng.region_step((i * nsched) // k if k < nsched else i % nsched, gs, isa, ibg, xl=True)
        eng.synchronize(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k
    for fu in ((1, 1, 1, 1), SDXL_FREEU):
        eng.set_freeu(*fu)
        run(warmup)
    off, on = [], []
    for _ in range(pairs):
        eng.set_freeu(1, 1, 1, 1)
        off.append(run(steps))
        eng.set_freeu(*SDXL_FREEU)
        on.append(run(steps))
    print(f"step, FreeU off: {' '.join(f'{v:.3f}' for v in off)} ms per step")
    print(f"step, FreeU on {SDXL_FREEU}: {' '.join(f'{v:.3f}' for v in on)} ms per step")
    print(f"difference of the means: {sum(on) / len(on) - sum(off) / len(off):+.3f} ms per step; spread of the off series "
          f"{max(off) - min(off):.3f} ms ({steps} steps per run, {pairs} alternated pairs, host clock around a device synchronise)")
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="also time bench.py's step with FreeU on against off (builds the SDXL engine)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    kernels()
    if a.step:
        step(a.steps, a.pairs)
