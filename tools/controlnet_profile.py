"""What a ControlNet (csrc/control.hip + the control copy of the encoder in csrc/engine.hip) costs at SDXL's 128 x 128 latents with the 7
streams of an injected rich-text step, all of them controlled.

  add       the residual add (rt_op_control_add) at the ten shapes a forward launches it at - the nine skips (128^2 x 320 three times,
            64^2 x 320, 64^2 x 640 twice, 32^2 x 640, 32^2 x 1280 twice) and the mid output (32^2 x 1280) -: HIP events over `launches`
            back-to-back calls, best of `reps`.  Bytes: the fp32 residual read once, the fp16 skip read and written once (8 per element);
            beside it a plain device-to-device copy that moves the same number of bytes (half of them read, half written), timed the
            same way on the same box.
  embedder  rt_set_control_hint on a 3 x 1024 x 1024 hint (channels 16, 32, 96, 256): host clock around the call, which synchronises
            and allocates its scratch - once per image, outside the step.
  step      (--step) bench.py's workload - SDXL, R = 4, inject_selfattn 0.5, 50-step Euler, seeded weights and inputs - with all seven
            streams controlled against the same step with every scale 0, in alternated pairs on one engine; and the algorithmic FLOPs
            of the step's MFMA launches (the engine's own per-launch count) with and without the control copy.
"""
import argparse
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ADD_SHAPES = ((128 * 128, 320),) * 3 + ((64 * 64, 320),) + ((64 * 64, 640),) * 2 + ((32 * 32, 640),) + ((32 * 32, 1280),) * 3


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


def add(B=7, launches=200, reps=5):
    import ctypes as C
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    streams, scales = (C.c_int * B)(*range(B)), (C.c_float * B)(*([1e-4] * B))      # a tiny scale: hundreds of in-place adds stay finite
    total = total_copy = 0.0
    for HW, Cc in sorted(set(ADD_SHAPES), reverse=True):
        n = ADD_SHAPES.count((HW, Cc))
        skip = torch.randn(B, HW, Cc, generator=g).half().to(dev)
        r = torch.randn(B, HW, Cc, generator=g).to(dev)
        src = torch.empty(B * HW * Cc * 4, dtype=torch.uint8, device=dev)           # 4 bytes read + 4 written per element = the add's 8
        dst = torch.empty_like(src)

        def op():
            rc = lib.rt_op_control_add(C.c_void_p(skip.data_ptr()), C.c_longlong(HW * Cc), Cc, C.c_void_p(r.data_ptr()), C.c_longlong(HW * Cc), Cc,
                                       streams, scales, B, B, HW, Cc, st)
            assert rc == 0, lib.rt_op_last_error().decode()
        for _ in range(3):
            op()
        t_add = _timed(op, launches, reps)
        t_copy = _timed(lambda: dst.copy_(src), launches, reps)
        by = 8.0 * B * HW * Cc
        assert bool(torch.isfinite(skip.float()).all())
        print(f"{HW} tokens x {Cc} channels, {B} streams ({n} per forward): add {t_add:.1f} us ({by / 1e6:.1f} MB, {by / t_add / 1e6:.2f} TB/s) | "
              f"device copy of the same bytes {t_copy:.1f} us ({by / t_copy / 1e6:.2f} TB/s)")
        total += n * t_add
        total_copy += n * t_copy
    print(f"all ten adds of a forward of {B} controlled streams: {total:.1f} us; the copies: {total_copy:.1f} us "
          f"(HIP events over {launches} back-to-back launches, best of {reps})")


def _sdxl_engine():
    from rich_text_to_image_amd.engine import SDXL_CONFIG, Engine
    dev = "cuda:0"
    eng = Engine(SDXL_CONFIG, 128, 128, device=0, max_streams=8, max_prompts=8, controlnet={})
    g = torch.Generator(device=dev).manual_seed(0)
    for name, shape in eng.weight_table():
        zero_conv = "controlnet_down_blocks" in name or "controlnet_mid_block" in name
        if name.endswith(".weight") and len(shape) >= 2:
            t = (torch.rand(shape, generator=g, device=dev) * 2 - 1) / math.sqrt(math.prod(shape[1:])) * (0.1 if zero_conv else 1.0)
        elif name.endswith(".weight"):
            t = 1.0 + 0.1 * (torch.rand(shape, generator=g, device=dev) * 2 - 1)
        else:
            t = 0.05 * (torch.rand(shape, generator=g, device=dev) * 2 - 1)
        eng.bind_weight(name, t)
        eng.synchronize()
        del t
    return eng


def embedder(eng, reps=5):
    hint = torch.rand(3, 1024, 1024, generator=torch.Generator().manual_seed(1)).to("cuda:0")
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        eng.set_control_hint(hint)
        ts.append((time.perf_counter() - t0) * 1e3)
    print(f"hint embedder, 3 x 1024 x 1024 -> [128 x 128, 320]: first call {ts[0]:.2f} ms, then {' '.join(f'{v:.2f}' for v in ts[1:])} ms "
          f"(host clock around rt_set_control_hint: eight fp32 convolution launches with the SiLU in their epilogue, scratch allocated and freed, one synchronise)")


def step(eng, steps=20, pairs=3, warmup=3):
    import bench
    dev = "cuda:0"
    R, hw, nsched, gs, isa, ibg = 4, 128, 50, 5.0, 0.5, 0.0
    inp = bench.synth_inputs(1000, R, hw, dev)
    ts, sig, init_sigma = bench.euler_tables(nsched)
    eng.set_prompts(inp["emb"], inp["pooled"], inp["tid"])
    eng.set_masks(inp["masks"])
    eng.set_fontsize(torch.tensor([5, 6]), torch.tensor([20.0, 20.0]))
    lat0 = (inp["lat"] * init_sigma).to(dev)
    P = inp["emb"].shape[0]
    on_scales, off_scales = [1.0] * P, [0.0] * P

    def run(k):
        eng.set_schedule(0, ts, sig, nsched)
        eng.set_latents(lat0)
        eng.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(k):
            eng.region_step((i * nsched) // k if k < nsched else i % nsched, gs, isa, ibg, xl=True)
        eng.synchronize(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k
    for sc in (off_scales, on_scales):
        eng.set_control_scales(sc)
        run(warmup)
    off, on = [], []
    for _ in range(pairs):
        eng.set_control_scales(off_scales)
        off.append(run(steps))
        eng.set_control_scales(on_scales)
        on.append(run(steps))
    print(f"step, every scale 0: {' '.join(f'{v:.3f}' for v in off)} ms per step")
    print(f"step, all seven streams controlled: {' '.join(f'{v:.3f}' for v in on)} ms per step")
    print(f"difference of the means: {sum(on) / len(on) - sum(off) / len(off):+.3f} ms per step; spread of the off series "
          f"{max(off) - min(off):.3f} ms ({steps} steps per run, {pairs} alternated pairs, host clock around a device synchronise)")
    flops = {}
    for label, sc in (("off", off_scales), ("on", on_scales)):
        eng.set_control_scales(sc)
        eng.set_schedule(0, ts, sig, nsched)
        eng.set_latents(lat0)
        eng.profile_enable(True)
        eng.region_step(0, gs, isa, ibg, xl=True)
        eng.synchronize()
        flops[label] = sum(v["total_flops"] for v in eng.profile_read().values())
        if label == "on":
            p = eng.profile_read_control()
            print(f"the adds inside that step: {p['launches']} launches, {p['total_ms'] * 1e3:.1f} us, {p['total_bytes'] / 1e6:.1f} MB "
                  f"({p['total_bytes'] / max(p['total_ms'], 1e-9) / 1e9:.2f} TB/s under per-launch events)")
        eng.profile_enable(False)
    print(f"algorithmic FLOPs of one injected step: {flops['off'] / 1e12:.2f} T without control, {flops['on'] / 1e12:.2f} T with all seven streams "
          f"controlled: the control copy adds {(flops['on'] - flops['off']) / 1e12:.2f} T = {(flops['on'] - flops['off']) / flops['off'] * 100:.1f} % of the UNet's")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="also time the embedder at 1024^2 and bench.py's step with control on against off (builds the SDXL engine)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    add()
    if a.step:
        e = _sdxl_engine()
        embedder(e)
        step(e, a.steps, a.pairs)
        e.close()
