"""What perturbed-attention guidance (csrc/pag.hip + the twin streams of csrc/step_driver.inl) costs at SDXL's 128 x 128 latents.

  identity  the identity attention (rt_op_identity_attention) at SDXL's mid block - 5 twins x 1024 tokens x 1280 channels (20 heads of
            64), V^T of 12 streams -: HIP events over `launches` back-to-back calls, best of `reps`.  Bytes: V^T read once, O written
            once (4 per element); beside it a plain device-to-device copy that moves the same number of bytes, timed the same way on
            the same box.
  fold      the fold of a step (rt_op_pag_fold) at 128 x 128 with 5 pairs of 12 streams: partner read and written, twin read (12 bytes
            per value), and the copy of the same bytes.
  step      (--step) bench.py's workload - SDXL, R = 4, inject_selfattn 0.5, 50-step Euler, seeded weights and inputs - with every
            conditional slot at sigma = 3 on the default layers (mid): 12 streams (7 + the twins of base, text_ref and three regions)
            against the same step with every sigma 0 (7 streams), in alternated pairs on one engine.
"""
import argparse
import ctypes as C
import math
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


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


def _copy_of(nbytes, launches, reps):
    src = torch.empty(int(nbytes) // 2, dtype=torch.uint8, device="cuda:0")      # half the bytes read, half written
    dst = torch.empty_like(src)
    return _timed(lambda: dst.copy_(src), launches, reps)


def identity(B=12, twins=5, H=20, N=1024, DP=64, launches=200, reps=5):
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    dev = "cuda:0"
    vt = torch.randn(H * DP, B * N, generator=torch.Generator().manual_seed(0)).bfloat16().to(dev)
    o = torch.zeros(B * N, H * DP, dtype=torch.bfloat16, device=dev)
    ent = (C.c_int * twins)(*range(B - twins, B))
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def op():
        rc = lib.rt_op_identity_attention(C.c_void_p(vt.data_ptr()), B * N, C.c_void_p(o.data_ptr()), H * DP, ent, twins, B, H, N, DP, st)
        assert rc == 0, lib.rt_op_last_error().decode()
    for _ in range(3):
        op()
    assert torch.equal(o[(B - twins) * N:], vt[:, (B - twins) * N:].t())
    t = _timed(op, launches, reps)
    by = 4.0 * twins * N * H * DP
    tc = _copy_of(by, launches, reps)
    print(f"identity attention, {twins} twins of {B} streams x {N} tokens x {H * DP} channels: {t:.1f} us ({by / 1e6:.1f} MB, {by / t / 1e6:.2f} TB/s) | "
          f"device copy of the same bytes {tc:.1f} us ({by / tc / 1e6:.2f} TB/s)  (HIP events over {launches} back-to-back launches, best of {reps})")


def fold(F=12, pairs=5, hw=128, launches=200, reps=5):
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    eps = torch.randn(F, hw * hw, 4, generator=torch.Generator().manual_seed(1)).to("cuda:0")
    s, tw = (C.c_int * pairs)(*range(1, 1 + pairs)), (C.c_int * pairs)(*range(F - pairs, F))
    rho = (C.c_float * pairs)(*([1e-4] * pairs))                                   # a tiny ratio: hundreds of in-place folds stay finite
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def op():
        rc = lib.rt_op_pag_fold(C.c_void_p(eps.data_ptr()), F, hw, hw, s, tw, rho, pairs, st)
        assert rc == 0, lib.rt_op_last_error().decode()
    for _ in range(3):
        op()
    t = _timed(op, launches, reps)
    by = 12.0 * pairs * hw * hw * 4
    tc = _copy_of(by, launches, reps)
    assert bool(torch.isfinite(eps).all())
    print(f"fold, {pairs} pairs of {F} streams at {hw} x {hw}: {t:.1f} us ({by / 1e6:.2f} MB, {by / t / 1e6:.2f} TB/s) | device copy of the same bytes "
          f"{tc:.1f} us ({by / tc / 1e6:.2f} TB/s)")


def _sdxl_engine():
    from rich_text_to_image_amd.engine import SDXL_CONFIG, Engine
    dev = "cuda:0"
    eng = Engine(SDXL_CONFIG, 128, 128, device=0, max_streams=12, max_prompts=8)
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
    return eng


def step(eng, steps=20, pairs=3, warmup=3):
    import bench
    from rich_text_to_image_amd.pag import resolve_layers
    dev = "cuda:0"
    R, hw, nsched, gs, isa, ibg = 4, 128, 50, 5.0, 0.5, 0.0
    inp = bench.synth_inputs(1000, R, hw, dev)
    ts, sig, init_sigma = bench.euler_tables(nsched)
    eng.set_prompts(inp["emb"], inp["pooled"], inp["tid"])
    eng.set_masks(inp["masks"])
    eng.set_fontsize(torch.tensor([5, 6]), torch.tensor([20.0, 20.0]))
    eng.set_pag_layers(resolve_layers(("mid",), eng.attn_modules()))
    lat0 = (inp["lat"] * init_sigma).to(dev)
    P = inp["emb"].shape[0]
    on_scales, off_scales = [0.0] + [3.0] * (P - 1), [0.0] * P

    def run(k):
        eng.set_schedule(0, ts, sig, nsched)
        eng.set_latents(lat0)
        eng.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(k):
            eng.region_step((i * nsched) // k if k < nsched else i % nsched, gs, isa, ibg, xl=True)
        eng.synchronize(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k
    counts = {}
    for label, sc in (("off", off_scales), ("on", on_scales)):
        eng.set_pag_scales(sc)
        eng.set_schedule(0, ts, sig, nsched)
        eng.set_latents(lat0)
        counts[label] = eng.region_step_part(0, gs, isa, ibg, True, 0, 1)[2][0]
        run(warmup)
    off, on = [], []
    for _ in range(pairs):
        eng.set_pag_scales(off_scales)
        off.append(run(steps))
        eng.set_pag_scales(on_scales)
        on.append(run(steps))
    print(f"step, every sigma 0 ({counts['off']} streams): {' '.join(f'{v:.3f}' for v in off)} ms per step")
    print(f"step, every conditional slot at sigma 3, layers mid ({counts['on']} streams): {' '.join(f'{v:.3f}' for v in on)} ms per step")
    m_on, m_off = sum(on) / len(on), sum(off) / len(off)
    print(f"ratio of the means {m_on / m_off:.3f} (stream ratio {counts['on'] / counts['off']:.3f}); spread of the off series {max(off) - min(off):.3f} ms "
          f"({steps} steps per run, {pairs} alternated pairs, host clock around a device synchronise)")
    eng.set_schedule(0, ts, sig, nsched)
    eng.set_latents(lat0)
    eng.profile_enable(True)
    eng.region_step(0, gs, isa, ibg, xl=True)
    eng.synchronize()
    p = eng.profile_read_pag()
    eng.profile_enable(False)
    print(f"the PAG launches inside that step: {p['launches']} launches, {p['total_ms'] * 1e3:.1f} us, {p['total_bytes'] / 1e6:.1f} MB (under per-launch events)")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="also time bench.py's step with PAG on against off (builds the SDXL engine)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    a = ap.parse_args()
    identity()
    fold()
    if a.step:
        e = _sdxl_engine()
        step(e, a.steps, a.pairs)
        e.close()
