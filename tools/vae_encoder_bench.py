"""VAE encoder (rt_vae_encode, RegionDiffusion.encode_imgs) against the decoder (rt_vae_decode) at the same image size and precision.

  python tools/vae_encoder_bench.py [--reps 10] [--warmup 2] [--out FILE]

For SD 512^2 and SDXL 1024^2, single pass and precise: one encoder and one decoder on random weights (the same init scheme as the
tests), each call warmed up, then encode and decode ALTERNATED in the same process, each timed on the host clock around a call that
ends in a stream synchronize (both C calls synchronize before they return).  Prints one JSON line per case: median / min ms of
each, their ratio, the FLOPs of each graph counted from the layer shapes (the contractions: convolutions, linears, attention
products) and the achieved TFLOP/s (FLOPs / median time; precise mode counts the one-pass FLOPs, it runs three MFMA passes).
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _conv(cin, cout, k, hw):
    return 2.0 * cin * cout * k * k * hw


def _res(cin, cout, hw):
    return _conv(cin, cout, 3, hw) + _conv(cout, cout, 3, hw) + (_conv(cin, cout, 1, hw) if cin != cout else 0.0)


def _attn(c, n):
    return 4 * 2.0 * n * c * c + 2 * 2.0 * n * n * c          # q, k, v, out projections + QK^T and PV


def encoder_flops(cfg, H, W):
    boc, lpb = cfg["block_out_channels"], cfg["layers_per_block"]
    hw = H * W
    f = _conv(3, boc[0], 3, hw)
    c = boc[0]
    for i, o in enumerate(boc):
        for j in range(lpb):
            f += _res(c if j == 0 else o, o, hw)
        c = o
        if i != len(boc) - 1:
            hw //= 4
            f += _conv(o, o, 3, hw)
    f += 2 * _res(c, c, hw) + _attn(c, hw)
    return f + _conv(c, 8, 3, hw) + _conv(8, 8, 1, hw)


def decoder_flops(cfg, h, w):
    boc, lpb = list(reversed(cfg["block_out_channels"])), cfg["layers_per_block"]
    hw = h * w
    f = _conv(4, 4, 1, hw) + _conv(4, boc[0], 3, hw)
    f += 2 * _res(boc[0], boc[0], hw) + _attn(boc[0], hw)
    c = boc[0]
    for i, o in enumerate(boc):
        for j in range(lpb + 1):
            f += _res(c if j == 0 else o, o, hw)
        c = o
        if i != len(boc) - 1:
            hw *= 4
            f += _conv(o, o, 3, hw)
    return f + _conv(c, 3, 3, hw)


def main():
    import torch
    from oracle.vae import random_vae_state_dict
    from rich_text_to_image_amd.engine import SD_VAE_CONFIG, SDXL_VAE_CONFIG, VaeDecoder, VaeEncoder
    from vae_encoder_ref import random_vae_encoder_state_dict
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=None, help="also append the JSON lines to this file")
    ap.add_argument("--cases", default="sd512,sdxl1024")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("vae_encoder_bench needs a GPU (no CPU timing is reported)")
    cases = {"sd512": ("SD", SD_VAE_CONFIG, 512), "sdxl1024": ("SDXL", SDXL_VAE_CONFIG, 1024)}
    for key in args.cases.split(","):
        name, cfg, size = cases[key]
        lat = size // 8
        cfgo = dict(cfg, latent_channels=4, out_channels=3)
        esd, dsd = random_vae_encoder_state_dict(cfgo, seed=0), random_vae_state_dict(cfgo, seed=0)
        g = torch.Generator().manual_seed(0)
        img = (torch.rand(1, 3, size, size, generator=g) * 2 - 1).cuda()
        z = torch.randn(1, 4, lat, lat, generator=g).cuda()
        for precise in (False, True):
            enc = VaeEncoder(cfg, lat, lat, device=0, state_dict=esd, precise=precise)
            dec = VaeDecoder(cfg, lat, lat, device=0, state_dict=dsd, precise=precise)
            for _ in range(args.warmup):
                enc.encode(img); dec.decode(z)
            te, td = [], []
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); enc.encode(img); torch.cuda.synchronize(); t1 = time.perf_counter()
                dec.decode(z); torch.cuda.synchronize(); t2 = time.perf_counter()
                te.append((t1 - t0) * 1e3); td.append((t2 - t1) * 1e3)
            fe, fd = encoder_flops(cfg, size, size), decoder_flops(cfg, lat, lat)
            me, md = statistics.median(te), statistics.median(td)
            line = {"case": f"{name} {size}^2", "precise": precise, "reps": args.reps,
                    "encode_ms_median": round(me, 3), "encode_ms_min": round(min(te), 3),
                    "decode_ms_median": round(md, 3), "decode_ms_min": round(min(td), 3),
                    "encode_over_decode": round(me / md, 3),
                    "encode_tflop": round(fe / 1e12, 3), "decode_tflop": round(fd / 1e12, 3), "work_ratio": round(fe / fd, 3),
                    "encode_tflops_per_s": round(fe / me / 1e9, 1), "decode_tflops_per_s": round(fd / md / 1e9, 1),
                    "device": torch.cuda.get_device_name(0)}
            print(json.dumps(line), flush=True)
            if args.out:
                with open(args.out, "a") as f:
                    f.write(json.dumps(line) + "\n")
            enc.close(); dec.close()


if __name__ == "__main__":
    main()
