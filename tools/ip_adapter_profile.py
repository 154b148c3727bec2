"""What the image-prompt term of attn2 (csrc/ipattn.hip, rt_op_ip_attention) costs at the two cross-attention shapes of an SDXL step at
128 x 128 latents with the 7 streams of an injected rich-text step, every stream carrying an image:

  7 x 1024 tokens x 20 heads x 64   (the 1280-channel level: 60 attn2 launches per forward)
  7 x 4096 tokens x 10 heads x 64   (the 640-channel level: 10 attn2 launches per forward)

with T = 4 and T = 16 image tokens.  HIP events over `launches` back-to-back calls, best of `reps`.  The launch is bound by bytes - Q read
once, O read and written once (the keys of a head are 4 KB) - so the rate those bytes give stands beside a plain device copy of the same
bytes (Q once, O twice = ONE copy launch of a buffer of 1.5 tensors) timed the same way on the same box.  Scales are tiny so that hundreds of in-place
applications stay finite: neither the arithmetic nor the traffic depends on the values.
Prints what it measured; writes the same lines to --out (profiles/ip_adapter_timing.txt)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = ((7, 1024, 20, 64, 60), (7, 4096, 10, 64, 10))      # streams, tokens, heads, DP, attn2 launches of this shape per SDXL forward


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


def main(launches=200, reps=5, out=None):
    import ctypes as C
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    dev = "cuda:0"
    g = torch.Generator().manual_seed(0)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    lines = []
    per_step = {4: 0.0, 16: 0.0}
    for (B, N, H, DP, per_forward) in SHAPES:
        HD = H * DP
        Q = (torch.randn(B * N, HD, generator=g) * DP ** -0.5 * 1.4426950408889634).to(torch.bfloat16).to(dev)
        O = torch.randn(B * N, HD, generator=g).to(torch.bfloat16).to(dev)
        K = torch.randn(8 * 16, HD, generator=g).to(torch.bfloat16).to(dev)
        VT = torch.randn(HD, 8 * 16, generator=g).to(torch.bfloat16).to(dev)
        src = torch.randn(3 * B * N * HD // 2, generator=g).to(torch.bfloat16).to(dev)      # 1.5 tensors read + written = the same bytes, one launch
        dst = torch.empty_like(src)
        slots = (C.c_int * B)(*[b % 8 for b in range(B)])
        scales = (C.c_float * B)(*([1e-4] * B))
        nbytes = 3.0 * B * N * HD * 2
        t_copy = _timed(lambda: dst.copy_(src), launches, reps)
        for T in (4, 16):
            counts = (C.c_int * B)(*([T] * B))

            def op():
                rc = lib.rt_op_ip_attention(C.c_void_p(Q.data_ptr()), HD, C.c_void_p(K.data_ptr()), HD, C.c_void_p(VT.data_ptr()), 8 * 16,
                                            C.c_void_p(O.data_ptr()), HD, slots, counts, scales, B, H, N, DP, st)
                assert rc == 0, lib.rt_op_last_error().decode()
            for _ in range(3):
                op()
            t = _timed(op, launches, reps)
            assert bool(torch.isfinite(O.float()).all())
            per_step[T] += per_forward * t
            lines.append(f"{B} x {N} tokens x {H} heads x {DP}, T = {T}: {t:.1f} us per launch ({nbytes / 1e6:.1f} MB of Q once + O twice, "
                         f"{nbytes / t / 1e6:.2f} TB/s) | device copy of the same bytes (one launch) {t_copy:.1f} us ({nbytes / t_copy / 1e6:.2f} TB/s) "
                         f"| the kernel reaches {t_copy / t:.2f} of the copy's rate")
    for T in (4, 16):
        lines.append(f"one SDXL forward of 7 streams, every stream with an image, T = {T}: 60 launches at 1024 tokens + 10 at 4096 = "
                     f"{per_step[T] / 1e3:.2f} ms per step")
    lines.append(f"(HIP events over {launches} back-to-back launches, best of {reps}; ONE form of the kernel for every shape: a wave owns a head and "
                 f"four 16-query tiles, the head's K / V^T fragments in registers, no LDS)")
    print("\n".join(lines))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.launches, a.reps, a.out)
