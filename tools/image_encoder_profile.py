"""What encoding a reference image costs (rich_text_to_image_amd/clip_vision_encoder.py) at the two encoders IP-Adapter ships with,
random weights: ViT-H/14 (width 1280, 16 heads of 80, 32 layers, MLP 5120) and ViT-bigG/14 (width 1664, 16 heads of 104, 48 layers,
MLP 8192), one and four 224 x 224 images (257 tokens each).  HIP events over `encodes` back-to-back encodes, best of `reps`; the share of
the attention launches is the time of L back-to-back rt_op_bidir_attention launches at the encoder's shape over the encode.  Beside
them two floors that are COMPUTED, not measured: the bf16 weight bytes read once at the 8 TB/s the HBM is specified for, and the
executed FLOP at the 2.5 PFLOP/s the dense bf16 MFMA is specified for.  For scale only (they solve different problems): the attention
launch at (1, 16, 257, 80) next to rt_op_causal_attention at its own largest shape (1, 16, 128, 80).
Prints what it measured; writes the same lines to --out (profiles/image_encoder_timing.txt)."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

ENCODERS = (("ViT-H/14", dict(hidden_size=1280, num_attention_heads=16, num_hidden_layers=32, intermediate_size=5120, hidden_act="gelu",
                             image_size=224, patch_size=14, projection_dim=1024)),
            ("ViT-bigG/14", dict(hidden_size=1664, num_attention_heads=16, num_hidden_layers=48, intermediate_size=8192, hidden_act="gelu",
                                image_size=224, patch_size=14, projection_dim=1280)))


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


def _attn(lib, fn, B, H, N, d):
    qkv = torch.randn(B * N, 3 * H * d, device="cuda:0").to(torch.bfloat16)
    out = torch.empty(B * N, H * d, device="cuda:0", dtype=torch.bfloat16)
    p = qkv.data_ptr()

    def op():
        rc = fn(C.c_void_p(p), C.c_void_p(p + 2 * H * d), C.c_void_p(p + 4 * H * d), 3 * H * d, C.c_void_p(out.data_ptr()), H * d, B, H, N, d,
                C.c_float(d ** -0.5), None)
        assert rc == 0, lib.rt_op_last_error().decode()
    return op, (qkv, out)


def main(encodes=5, reps=3, out=None):
    from make_image_encoder import random_state_dict
    from rich_text_to_image_amd.clip_vision_encoder import HipCLIPVisionEncoder
    from rich_text_to_image_amd.engine import load_library
    lib = load_library()
    lines = []
    for name, cfg in ENCODERS:
        Cc, H, L, I, P = cfg["hidden_size"], cfg["num_attention_heads"], cfg["num_hidden_layers"], cfg["intermediate_size"], cfg["projection_dim"]
        N, d = 257, Cc // H
        enc = HipCLIPVisionEncoder(random_state_dict(cfg, device="cuda:0"), cfg, device=0)
        wbytes = sum(t.numel() * t.element_size() for t in enc.parameter_tensors() if t.dtype == torch.bfloat16)
        for B in (1, 4):
            px = torch.randint(0, 256, (B, 224, 224, 3), dtype=torch.uint8, device="cuda:0")
            o = enc(px)
            assert bool(torch.isfinite(o.image_embeds).all())
            t_enc = _timed(lambda: enc(px), encodes, reps)              # includes the synchronize at the end of every encode
            op, keep = _attn(lib, lib.rt_op_bidir_attention, B, H, N, d)
            op()
            t_att = _timed(op, 50, reps)
            M = B * N
            flop = L * (2.0 * M * Cc * (4 * Cc + 2 * I) + 4.0 * B * H * N * N * d) + 2.0 * B * (N - 1) * Cc * 588 + 2.0 * B * Cc * P
            lines.append(f"{name}, {B} image(s): {t_enc / 1e3:.2f} ms per encode; the {L} attention launches {L * t_att / 1e3:.2f} ms = "
                         f"{100 * L * t_att / t_enc:.1f} % ({t_att:.1f} us each at ({B}, {H}, {N}, {d})) | floors, computed not measured: "
                         f"{wbytes / 1e9:.2f} GB of bf16 weights read once at 8 TB/s = {wbytes / 8e12 * 1e3:.2f} ms; {flop / 1e12:.2f} TFLOP executed at "
                         f"2.5 PFLOP/s = {flop / 2.5e15 * 1e3:.2f} ms")
        del enc
        torch.cuda.empty_cache()
    op, keep = _attn(lib, lib.rt_op_bidir_attention, 1, 16, 257, 80)
    op()
    t_b = _timed(op, 200, reps)
    op2, keep2 = _attn(lib, lib.rt_op_causal_attention, 1, 16, 128, 80)
    op2()
    t_c = _timed(op2, 200, reps)
    lines.append(f"for scale only: rt_op_bidir_attention (1, 16, 257, 80) {t_b:.1f} us; rt_op_causal_attention at its largest shape (1, 16, 128, 80) {t_c:.1f} us "
                 f"(a quarter of the score products, causal, one thread per query: a different problem)")
    lines.append(f"(HIP events over {encodes} back-to-back encodes / 50 - 200 back-to-back launches, best of {reps}; an encode = patchify, the patch GEMM, the front "
                 f"end, L x (2 LayerNorms, 4 GEMMs, attention, activation), the pooled LayerNorm and projection, and one synchronize)")
    print("\n".join(lines))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--encodes", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    main(a.encodes, a.reps, a.out)
