"""Cost of prompts longer than one 77-token CLIP window (python tools/long_prompt_bench.py [--steps 10] [--rounds 3] [--out FILE]).

1. Step cost: SDXL at 1024 x 1024 (128 x 128 latent), 4 regions, injected schedule as bench.py times it - the BASE prompt at 77, 154 and
   231 keys, the negative and the region prompts at 77.  One engine (max_keys = 231), the variants alternate inside every round, ms per
   step = median over the rounds.  The 77-key variant launches what a default engine launches.
2. The cross-attention launch alone (rt_op_attention_keys, HIP events): 7 streams x 1024 tokens x 20 heads and 7 x 4096 x 10 heads,
   d = 64, two of the seven streams at 77 / 154 / 231 keys (base and text_ref carry the base prompt), the rest at 77.

3. --kernel_ab KEYS TOKENS HEADS: the kernel A/B, meant to run under `rocprofv3 --kernel-trace --stats -- python tools/long_prompt_bench.py
   --kernel_ab ...` (a run of its own per case): 7 streams, all at KEYS (154 / 231) keys, d = 64, 30 launches of crossmw_kernel and 30 of
   attn_kernel<CROSS> (debug bit 19) alternating; the trace's per-kernel statistics are the result (profiles/long_prompt_kernels.txt).

Prints one JSON object; --out also writes it to a file.  The figures of 2. are times of the whole host call (one to five launches with
their gaps), not kernel times."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from bench import euler_tables, synth_inputs  # noqa: E402


def step_cost(steps, rounds):
    from rich_text_to_image_amd.engine import Engine, SDXL_CONFIG
    R, hw, nsched, gs, isa = 4, 128, 50, 5.0, 0.5
    dev = "cuda:0"
    eng = Engine(SDXL_CONFIG, hw, hw, device=0, max_streams=8, max_prompts=8, max_keys=231)
    eng.init_random_weights(seed=0)
    inp = synth_inputs(1000, R, hw, dev)
    ts, sig, init_sigma = euler_tables(nsched)
    g = torch.Generator().manual_seed(5)
    emb = torch.zeros(R + 1, 231, 2048, device=dev)
    emb[:, :77] = inp["emb"]
    emb[R, 77:] = torch.randn(154, 2048, generator=g).to(dev)          # the base prompt's second and third window
    eng.set_masks(inp["masks"])
    eng.set_fontsize(torch.tensor([5, 6]), torch.tensor([20.0, 20.0]))
    lat0 = (inp["lat"] * init_sigma).to(dev)
    times = {77: [], 154: [], 231: []}
    for r in range(rounds + 1):                                         # round 0 warms every variant
        for keys in (77, 154, 231):
            eng.set_prompts(emb, inp["pooled"], inp["tid"], key_counts=[77] * R + [keys])
            eng.set_schedule(0, ts, sig, nsched)
            eng.set_latents(lat0)
            eng.synchronize()
            t0 = time.perf_counter()
            for i in range(steps):
                eng.region_step((i * nsched) // steps, gs, isa, 0.0, xl=True)
            eng.synchronize()
            if r:
                times[keys].append((time.perf_counter() - t0) * 1e3 / steps)
            assert torch.isfinite(eng.read_latents(hw, hw)).all()
    eng.close()
    return {str(k): dict(ms_per_step=statistics.median(v), rounds=[round(x, 3) for x in v]) for k, v in times.items()}


def kernel_cost(reps=20):
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    dev, out = "cuda:0", {}
    for N, H in ((1024, 20), (4096, 10)):
        B, P, KP, DP = 7, 5, 288, 64
        g = torch.Generator().manual_seed(1)
        Q = torch.randn(B * N, H * DP, generator=g).to(dev).to(torch.bfloat16)
        K = torch.randn(P * KP, H * DP, generator=g).to(dev).to(torch.bfloat16)
        VT = torch.randn(H * DP, P * KP, generator=g).to(dev).to(torch.bfloat16)
        O = torch.empty_like(Q)
        wabs, wsgn = torch.ones(2, KP, device=dev), torch.ones(2, KP, device=dev)
        prompt = [0, 4, 0, 4, 1, 2, 3]                                   # [uncond, base, uncond_ref, text_ref, regions...]
        wset = [-1, 1, -1, -1, -1, -1, -1]
        ia = lambda v: (C.c_int * B)(*v)
        for keys in (77, 154, 231):
            counts = [keys if p == 4 else 77 for p in prompt]
            ms = []
            for it in range(reps + 3):
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                rc = lib.rt_op_attention_keys(C.c_void_p(Q.data_ptr()), Q.stride(0), C.c_void_p(K.data_ptr()), K.stride(0), C.c_void_p(VT.data_ptr()),
                                              VT.stride(0), C.c_void_p(O.data_ptr()), O.stride(0), None, ia(prompt), ia(wset), C.c_void_p(wabs.data_ptr()),
                                              C.c_void_p(wsgn.data_ptr()), ia(counts), B, H, N, KP, DP, None)
                b.record()
                torch.cuda.synchronize()
                assert rc == 0, lib.rt_op_last_error().decode()
                if it >= 3:
                    ms.append(a.elapsed_time(b) * 1e3)
            out[f"{B}x{N}x{H}h keys={keys}"] = dict(us_median=round(statistics.median(ms), 2), us_min=round(min(ms), 2), us_max=round(max(ms), 2))
    return out


def kernel_ab(keys, N, H, reps=30):
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    dev, B, P, KP, DP = "cuda:0", 7, 5, 288, 64
    g = torch.Generator().manual_seed(1)
    Q = torch.randn(B * N, H * DP, generator=g).to(dev).to(torch.bfloat16)
    K = torch.randn(P * KP, H * DP, generator=g).to(dev).to(torch.bfloat16)
    VT = torch.randn(H * DP, P * KP, generator=g).to(dev).to(torch.bfloat16)
    O = torch.empty_like(Q)
    wabs, wsgn = torch.ones(2, KP, device=dev), torch.ones(2, KP, device=dev)
    ia = lambda v: (C.c_int * B)(*v)
    prompt, wset, counts = [0, 4, 0, 4, 1, 2, 3], [-1, 1, -1, -1, -1, -1, -1], [keys] * B
    for it in range(2 * (reps + 3)):
        lib.rt_op_gemm_debug((1 << 19) if it & 1 else 0)                 # odd launches: the generic tile loop
        rc = lib.rt_op_attention_keys(C.c_void_p(Q.data_ptr()), Q.stride(0), C.c_void_p(K.data_ptr()), K.stride(0), C.c_void_p(VT.data_ptr()),
                                      VT.stride(0), C.c_void_p(O.data_ptr()), O.stride(0), None, ia(prompt), ia(wset), C.c_void_p(wabs.data_ptr()),
                                      C.c_void_p(wsgn.data_ptr()), ia(counts), B, H, N, KP, DP, None)
        assert rc == 0, lib.rt_op_last_error().decode()
        torch.cuda.synchronize()
    lib.rt_op_gemm_debug(0)
    print(json.dumps(dict(kernel_ab=dict(keys=keys, tokens=N, heads=H, streams=B, launches_each=reps + 3))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel_ab", type=int, nargs=3, default=None, metavar=("KEYS", "TOKENS", "HEADS"))
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.kernel_ab:
        return kernel_ab(*a.kernel_ab)
    res = dict(workload="SDXL 1024x1024, 4 regions, inject_selfattn 0.5; base prompt keys 77 / 154 / 231, other prompts 77",
               device=torch.cuda.get_device_name(0), steps_per_round=a.steps, step=step_cost(a.steps, a.rounds), cross_attention_call=kernel_cost())
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
