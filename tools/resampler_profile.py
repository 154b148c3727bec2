"""What the Resampler of an IP-Adapter "plus" checkpoint costs (rich_text_to_image_amd/resampler.py, csrc/resampler.hip), random weights.
HIP events over back-to-back launches, best of `reps`, as tools/image_encoder_profile.py.

  rt_op_latent_attention at (B, H, Nq, Nk, d) = (1, 12, 16, 273, 64) (SD-v1.5 plus) and (1, 20, 16, 273, 64) (SDXL plus), and for 4 images;
  the whole Resampler at the two published geometries - ip-adapter-plus_sd15: E 1280, dim 768, 12 heads of 64, 4 layers, 16 tokens, D 768;
  ip-adapter-plus_sdxl_vit-h: E 1280, dim 1280, 20 heads of 64, 4 layers, 16 tokens, D 2048 - over 257 hidden states, 1 and 4 images.

Beside each figure a floor that is COMPUTED, not measured, at the 8 TB/s the HBM is specified for: the K and V bytes read once (kernel),
the bf16 weight bytes read once (Resampler; a call of B images runs its GEMMs image by image, the floor counts the weights once).
Prints what it measured; writes the same lines to --out (profiles/resampler_timing.txt)."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))

# (name, E, dim, dim_head, heads, T, depth, D)
RESAMPLERS = (("ip-adapter-plus_sd15", 1280, 768, 64, 12, 16, 4, 768), ("ip-adapter-plus_sdxl_vit-h", 1280, 1280, 64, 20, 16, 4, 2048))
KERNEL_SHAPES = ((1, 12, 16, 273, 64), (1, 20, 16, 273, 64), (4, 12, 16, 273, 64), (4, 20, 16, 273, 64))


def _timed(fn, n, reps):
    best = float("inf")
    for _ in range(reps):
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(n):
            fn()
        b.record()
        torch.cuda.synchronize()
        best = min(best, a.elapsed_time(b) * 1e3 / n)
    return best                                                         # us per call


def main(calls=10, reps=3, out=None):
    import resampler_ref as RS
    from rich_text_to_image_amd.engine import load_library
    from rich_text_to_image_amd.resampler import HipResampler, check_resampler
    lib = load_library()
    lines = []
    for B, H, Nq, Nk, d in KERNEL_SHAPES:
        q = torch.randn(B * Nq, H * d, device="cuda:0").to(torch.bfloat16)
        kv = torch.randn(B * Nk, 2 * H * d, device="cuda:0").to(torch.bfloat16)
        o = torch.empty(B * Nq, H * d, device="cuda:0", dtype=torch.bfloat16)

        def op():
            rc = lib.rt_op_latent_attention(C.c_void_p(q.data_ptr()), H * d, C.c_void_p(kv.data_ptr()), C.c_void_p(kv.data_ptr() + 2 * H * d), 2 * H * d,
                                            C.c_void_p(o.data_ptr()), H * d, B, H, Nq, Nk, d, C.c_float(d ** -0.5), None)
            assert rc == 0, lib.rt_op_last_error().decode()
        op()
        t = _timed(op, 200, reps)
        kvb = kv.numel() * 2
        lines.append(f"rt_op_latent_attention ({B}, {H}, {Nq}, {Nk}, {d}): {t:.1f} us per launch, {B * H} workgroups | floor, computed not measured: "
                     f"{kvb / 1e3:.0f} KB of K and V read once at 8 TB/s = {kvb / 8e12 * 1e6:.2f} us")
    for name, E, dim, dh, heads, T, depth, D in RESAMPLERS:
        rs = HipResampler(check_resampler(RS.random_resampler(E, dim, dh, heads, T, depth, D, seed=1), dh), device=0)
        wbytes = sum(t.numel() * t.element_size() for t in rs.parameter_tensors() if t.dtype == torch.bfloat16)
        for B in (1, 4):
            h = RS.hidden_inputs(B, 257, E, seed=2).to("cuda:0")
            assert bool(torch.isfinite(rs(h)).all())
            t = _timed(lambda: rs(h), calls, reps)                      # includes the synchronize at the end of every call
            lines.append(f"{name} Resampler, {B} image(s) of 257 hidden states: {t / 1e3:.2f} ms per call ({3 + 2 * B + depth * (6 * B + 5)} launches) | "
                         f"floor, computed not measured: {wbytes / 1e6:.1f} MB of bf16 weights read once at 8 TB/s = {wbytes / 8e12 * 1e6:.1f} us")
        del rs
        torch.cuda.empty_cache()
    lines.append(f"(HIP events over 200 back-to-back kernel launches / {calls} back-to-back Resampler calls, best of {reps}; a call = the cast, proj_in, per layer "
                 f"2 + B LayerNorms, a row copy, 5 B GEMMs, the attention and the GELU, then the cast, proj_out and norm_out, and one synchronize)")
    print("\n".join(lines))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.calls, a.reps, a.out)
