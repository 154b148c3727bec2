"""What the regional LoRA term (csrc/lora.hip, rt_op_lora_add) costs.

  op    the launch at SDXL's two attention widths on a 128 x 128 latent with the 7 streams of an injected rich-text step -
        7 x 1024 rows x 1280 and 7 x 4096 rows x 640 (K = N: to_q / to_out; bf16 row-major) - at R = 16 / 64 / 128 rank columns with 1 and
        with 7 adapted streams.  HIP events over `launches` back-to-back calls, best of `reps`.  The launch is bound by bytes - X read once,
        Y read and written once, the factors stay in L2 - so a plain device copy of the same bytes (ONE launch of a buffer of 1.5
        tensors), timed the same way on the same box, stands beside every figure.  Scales are tiny so that hundreds of in-place
        applications stay finite: neither the arithmetic nor the traffic depends on the values.
  step  (--step) bench.py's workload - SDXL, R = 4 regions, inject_selfattn 0.5, 50-step Euler, seeded weights and inputs - on an engine
        with lora_rank = 64: one region adapted and all seven streams adapted against the same engine with every scale 0, in
        alternated pairs, host clock around a device synchronise.
  ff    (--ff) ff.net.0.proj's kernel (rt_op_lora_geglu) at 7 x 4096 rows with C = 640 and 7 x 1024 rows with C = 1280, the same ranks and
        stream counts, beside a device copy of its bytes (Z read, X read, out written); an adapted stream's whole ff.net.0.proj - LayerNorm,
        the plain weight into fp32, the kernel - beside the fused GEGLU launch for the same rows; and the fp16-trunk launch (rt_op_lora_add,
        form 2) at ff.net.2's K = 4C.  With --ff, --step times the engine with lora_targets = 1 (adapters on all twelve module kinds)
        and the engine with lora_targets = 0 (the eight attention projections), each against its own scale-0 series.
Prints what it measured; --out also writes the lines to a file (profiles/regional_lora_timing.txt, profiles/regional_lora_ff_timing.txt)."""
import argparse
import math
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ((7, 1024, 1280), (7, 4096, 640))      # streams, rows per stream, K = N
LINES = []


def say(s):
    print(s, flush=True)
    LINES.append(s)


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


def op(launches=200, reps=5):
    import ctypes as C
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for (B, rows, W) in SHAPES:
        X = torch.randn(B * rows, W, generator=g).to(torch.bfloat16).to(dev)
        Y = torch.randn(B * rows, W, generator=g).to(torch.bfloat16).to(dev)
        for nact in (1, B):
            nbytes = 3.0 * nact * rows * W * 2
            src = torch.randn(3 * nact * rows * W // 2, generator=g).to(torch.bfloat16).to(dev)      # 1.5 tensors read + written = the same bytes
            dst = torch.empty_like(src)
            t_copy = _timed(lambda: dst.copy_(src), launches, reps)
            for R in (16, 64, 128):
                down = (torch.randn(R, W, generator=g) / math.sqrt(W)).to(torch.bfloat16).to(dev)
                up = (torch.randn(W, R, generator=g) / math.sqrt(R)).to(torch.bfloat16).to(dev)
                aor = torch.ones(R, device=dev)
                col = torch.zeros(R, dtype=torch.int32, device=dev)
                rows_at = (C.c_int * B)(*[b * rows for b in range(B)])
                sc = (C.c_float * (4 * B))(*[1e-4 if (l == 0 and b < nact) else 0.0 for b in range(B) for l in range(4)])
                n = C.c_int(0)

                def launch():
                    rc = lib.rt_op_lora_add(C.c_void_p(X.data_ptr()), W, C.c_void_p(down.data_ptr()), W, C.c_void_p(up.data_ptr()), R,
                                            C.c_void_p(aor.data_ptr()), C.c_void_p(col.data_ptr()), C.c_void_p(Y.data_ptr()), W, 0, rows_at, sc,
                                            B, rows, W, W, R, C.byref(n), st)
                    assert rc == 0, lib.rt_op_last_error().decode()
                for _ in range(3):
                    launch()
                assert n.value == nact
                t = _timed(launch, launches, reps)
                assert bool(torch.isfinite(Y.float()).all())
                flops = 4.0 * nact * rows * R * W
                say(f"{nact} of {B} streams x {rows} rows x {W}, R = {R}: {t:.1f} us per launch ({nbytes / 1e6:.1f} MB of X once + Y twice, {nbytes / t / 1e6:.2f} TB/s, "
                    f"{flops / t / 1e6:.1f} TFLOP/s) | device copy of the same bytes (one launch) {t_copy:.1f} us ({nbytes / t_copy / 1e6:.2f} TB/s) "
                    f"| the kernel reaches {t_copy / t:.2f} of the copy's rate")
    say(f"(HIP events over {launches} back-to-back launches, best of {reps}; ONE kernel family: a wave owns 32 rows of one stream and chains both "
        f"products in registers, no LDS, no barrier; the factors are re-read from L2 by every wave)")


def ff(launches=100, reps=5):
    import ctypes as C
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    for (B, rows, W) in ((7, 4096, 640), (7, 1024, 1280)):
        N = 8 * W
        X = torch.randn(B * rows, W, generator=g).to(torch.bfloat16).to(dev)
        Z = torch.randn(B * rows, N, device=dev)
        out = torch.empty(B * rows, N // 2, dtype=torch.bfloat16, device=dev)
        rows_at = (C.c_int * B)(*[b * rows for b in range(B)])
        aor = torch.ones(128, device=dev)
        col = torch.zeros(128, dtype=torch.int32, device=dev)
        for nact in (1, B):
            nbytes = nact * rows * (4.0 * N + 2.0 * W + 2.0 * N / 2)
            src = torch.empty(int(nbytes) // 4, dtype=torch.bfloat16, device=dev).normal_()      # half the bytes read, half written
            dst = torch.empty_like(src)
            t_copy = _timed(lambda: dst.copy_(src), launches, reps)
            sc = (C.c_float * (4 * B))(*[0.5 if (l == 0 and b < nact) else 0.0 for b in range(B) for l in range(4)])
            for R in (16, 64, 128):
                down = (torch.randn(R, W, generator=g) / math.sqrt(W)).to(torch.bfloat16).to(dev)
                up = (torch.randn(N, R, generator=g) / math.sqrt(R)).to(torch.bfloat16).to(dev)
                n = C.c_int(0)

                def launch():
                    rc = lib.rt_op_lora_geglu(p(X), W, p(down), W, p(up), R, p(aor), p(col), p(Z), N, p(out), N // 2, rows_at, sc, B, rows, W, N, R, C.byref(n), st)
                    assert rc == 0, lib.rt_op_last_error().decode()
                for _ in range(3):
                    launch()
                assert n.value == nact
                t = _timed(launch, launches, reps)
                say(f"lora_geglu, {nact} of {B} streams x {rows} rows, C = {W}, R = {R}: {t:.1f} us per launch ({nbytes / 1e6:.1f} MB: Z and X read, out written; "
                    f"{nbytes / t / 1e6:.2f} TB/s, {2.0 * nact * rows * R * (W + N) / t / 1e6:.1f} TFLOP/s) | device copy of the same bytes {t_copy:.1f} us "
                    f"({nbytes / t_copy / 1e6:.2f} TB/s) | the kernel reaches {t_copy / t:.2f} of the copy's rate")
        # one adapted stream's whole ff.net.0.proj beside the fused launch for the same rows
        h = torch.randn(rows, W, generator=g).to(torch.float16).to(dev)
        gam, bet, bias = torch.ones(W, device=dev), torch.zeros(W, device=dev), torch.zeros(N, device=dev)
        Wt = (torch.randn(N, W, generator=g) / math.sqrt(W)).to(torch.bfloat16).to(dev)
        xn = torch.empty(rows, W, dtype=torch.bfloat16, device=dev)
        one = (C.c_float * 4)(0.5, 0, 0, 0)
        zero = (C.c_int * 1)(0)
        for R in (16, 64, 128):
            down = (torch.randn(R, W, generator=g) / math.sqrt(W)).to(torch.bfloat16).to(dev)
            up = (torch.randn(N, R, generator=g) / math.sqrt(R)).to(torch.bfloat16).to(dev)

            def ln():
                assert lib.rt_op_layernorm_f16(p(h), p(gam), p(bet), p(xn), rows, W, C.c_float(1e-5), st) == 0

            def gemm(epi, o, ldo):
                assert lib.rt_op_gemm(p(xn), p(Wt), p(bias), p(o), None, None, 0, epi, rows, N, W, W, W, ldo, 0, 0, rows, 0, 0, 0, 0, 0, st) == 0, lib.rt_op_last_error().decode()

            def kern():
                assert lib.rt_op_lora_geglu(p(xn), W, p(down), W, p(up), R, p(aor), p(col), p(Z), N, p(out), N // 2, zero, one, 1, rows, W, N, R, None, st) == 0

            def unfused():
                ln(); gemm(1, Z, N); kern()
            for f in (unfused, lambda: gemm(3, out, N // 2)):
                f()
            t_ln, t_g32, t_k = _timed(ln, launches, reps), _timed(lambda: gemm(1, Z, N), launches, reps), _timed(kern, launches, reps)
            t_un, t_fu = _timed(unfused, launches, reps), _timed(lambda: gemm(3, out, N // 2), launches, reps)
            say(f"ff.net.0.proj of ONE adapted stream, {rows} rows, C = {W}, R = {R}: LayerNorm {t_ln:.1f} + fp32 GEMM {t_g32:.1f} + lora_geglu {t_k:.1f} us alone, "
                f"{t_un:.1f} us back to back | the fused GEGLU GEMM for the same rows {t_fu:.1f} us (plain weight on normalised rows; the engine's folded "
                f"form also saves the LayerNorm launch) | unfused / fused = {t_un / t_fu:.2f}")
        # the fp16-trunk launch at ff.net.2's K = 4C
        X4 = torch.randn(B * rows, 4 * W, generator=g).to(torch.bfloat16).to(dev)
        Y = torch.randn(B * rows, W, generator=g).to(torch.float16).to(dev)
        for nact in (1, B):
            nbytes = nact * rows * (2.0 * 4 * W + 2 * 2.0 * W)
            src = torch.empty(int(nbytes) // 4, dtype=torch.bfloat16, device=dev).normal_()
            dst = torch.empty_like(src)
            t_copy = _timed(lambda: dst.copy_(src), launches, reps)
            sc = (C.c_float * (4 * B))(*[1e-4 if (l == 0 and b < nact) else 0.0 for b in range(B) for l in range(4)])
            for R in (16, 64, 128):
                down = (torch.randn(R, 4 * W, generator=g) / math.sqrt(4 * W)).to(torch.bfloat16).to(dev)
                up = (torch.randn(W, R, generator=g) / math.sqrt(R)).to(torch.bfloat16).to(dev)

                def launch():
                    rc = lib.rt_op_lora_add(p(X4), 4 * W, p(down), 4 * W, p(up), R, p(aor), p(col), p(Y), W, 2, rows_at, sc, B, rows, 4 * W, W, R, None, st)
                    assert rc == 0, lib.rt_op_last_error().decode()
                for _ in range(3):
                    launch()
                t = _timed(launch, launches, reps)
                say(f"lora_add fp16 trunk at ff.net.2, {nact} of {B} streams x {rows} rows, K = {4 * W}, N = {W}, R = {R}: {t:.1f} us per launch ({nbytes / 1e6:.1f} MB, "
                    f"{nbytes / t / 1e6:.2f} TB/s) | device copy of the same bytes {t_copy:.1f} us | the kernel reaches {t_copy / t:.2f} of the copy's rate")
        del X, Z, out, X4, Y
    say(f"(HIP events over {launches} back-to-back launches, best of {reps})")


def _sdxl_engine(rank, targets=0):
    from rich_text_to_image_amd.engine import SDXL_CONFIG, Engine
    dev = "cuda:0"
    eng = Engine(SDXL_CONFIG, 128, 128, device=0, max_streams=8, max_prompts=8, lora_rank=rank, lora_targets=targets)
    g = torch.Generator(device=dev).manual_seed(0)
    for name, shape in eng.weight_table():
        if name.endswith(".alpha_over_rank"):
            t = torch.ones(shape, device=dev)
        elif name.endswith(".weight") and len(shape) >= 2:
            t = (torch.rand(shape, generator=g, device=dev) * 2 - 1) / math.sqrt(math.prod(shape[1:])) * (0.1 if name.startswith("lora.") else 1.0)
        elif name.endswith(".weight"):
            t = 1.0 + 0.1 * (torch.rand(shape, generator=g, device=dev) * 2 - 1)
        else:
            t = 0.05 * (torch.rand(shape, generator=g, device=dev) * 2 - 1)
        eng.bind_weight(name, t)
        eng.synchronize()
        del t
    return eng


def step(rank=64, steps=20, pairs=3, warmup=3, targets=0):
    import ctypes as C
    import bench
    eng = _sdxl_engine(rank, targets)
    dev = "cuda:0"
    R, hw, nsched, gs, isa, ibg = 4, 128, 50, 5.0, 0.5, 0.0
    inp = bench.synth_inputs(1000, R, hw, dev)
    ts, sig, init_sigma = bench.euler_tables(nsched)
    eng.set_prompts(inp["emb"], inp["pooled"], inp["tid"])
    eng.set_masks(inp["masks"])
    eng.set_fontsize(torch.tensor([5, 6]), torch.tensor([20.0, 20.0]))
    lat0 = (inp["lat"] * init_sigma).to(dev)
    P = inp["emb"].shape[0]
    series = {"every scale 0": [(0.0,)] * P, "one region adapted": [(0.0,)] + [(0.5,)] + [(0.0,)] * (P - 2), "all seven streams adapted": [(0.5,)] * P}

    def run(k):
        eng.set_schedule(0, ts, sig, nsched)
        eng.set_latents(lat0)
        eng.synchronize(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for i in range(k):
            eng.region_step((i * nsched) // k if k < nsched else i % nsched, gs, isa, ibg, xl=True)
        eng.synchronize(); torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3 / k
    for sc in series.values():
        eng.set_lora_scales(sc)
        run(warmup)
    got = {k: [] for k in series}
    for _ in range(pairs):
        for k, sc in series.items():
            eng.set_lora_scales(sc)
            got[k].append(run(steps))
    for k, v in got.items():
        say(f"step, lora_rank {rank}, lora_targets {targets}, {k}: {' '.join(f'{x:.3f}' for x in v)} ms per step (mean {sum(v) / len(v):.3f})")
    off = got["every scale 0"]
    say(f"spread of the scale-0 series {max(off) - min(off):.3f} ms ({steps} steps per run, {pairs} alternated triples, host clock around a device synchronise)")
    eng.set_lora_scales(series["all seven streams adapted"])
    eng.set_schedule(0, ts, sig, nsched)
    eng.set_latents(lat0)
    eng.profile_enable(True)
    eng.region_step(0, gs, isa, ibg, xl=True)
    eng.synchronize()
    n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
    assert eng.lib.rt_profile_read2(eng.h, 9, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)) == 0
    eng.profile_enable(False)
    say(f"the adapter launches inside that step: {n.value} launches, {ms.value:.3f} ms, {by.value / 1e6:.1f} MB, {fl.value / 1e9:.1f} GFLOP "
        f"({by.value / max(ms.value, 1e-9) / 1e9:.2f} TB/s under per-launch events; the LayerNorm-rows and partials launches of the folded layers are not in this class)")
    eng.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true", help="also time bench.py's step with adapters on against off (builds the SDXL engine)")
    ap.add_argument("--rank", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--ff", action="store_true", help="the feed-forward kernel and ff.net.2's launch instead of the attention shapes; with --step both target sets")
    a = ap.parse_args()
    if a.ff:
        ff()
    else:
        op()
    if a.step:
        for targets in ((1, 0) if a.ff else (0,)):
            step(a.rank, a.steps, a.pairs, targets=targets)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
