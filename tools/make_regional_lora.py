"""Writes a synthetic regional-LoRA checkpoint for one of the tiny UNet configs (oracle/unet.py): nothing real is at hand offline, and
the tests and the command-line round trip need a file in a real layout.

  python tools/make_regional_lora.py out.safetensors --config xl --rank 4 --alpha 2 --layout kohya --seed 1 --gain 2

The factors adapt the eight attention projections of every transformer block - with --targets transformer also ff.net.0.proj, ff.net.2,
proj_in and proj_out, kohya's default network (load it with targets="transformer" / --region_lora_targets transformer) -: down uniform(+-1 / sqrt(K)), up uniform(+-gain / sqrt(rank)),
so that at alpha = rank the delta is `gain` times the size of the weights it is added to - far above the forward bar of the tests.
--layout: kohya (lora_unet_..., with .alpha), peft (lora_A / lora_B), diffusers (>= 0.20: .lora.down / .lora.up), diffusers018
(attention-processor names; attention only).  --unet_seed is the seed of oracle.unet.random_state_dict the adapter is meant for (shapes only)."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("out")
    p.add_argument("--config", choices=("sd", "xl"), default="xl")
    p.add_argument("--rank", type=int, default=4)
    p.add_argument("--alpha", type=float, default=None, help="kohya layout only (default: rank)")
    p.add_argument("--layout", choices=("kohya", "peft", "diffusers", "diffusers018"), default="kohya")
    p.add_argument("--seed", type=int, default=1)
    p.add_argument("--gain", type=float, default=2.0)
    p.add_argument("--unet_seed", type=int, default=11)
    p.add_argument("--targets", choices=("attention", "transformer"), default="attention")
    a = p.parse_args(argv)
    if a.targets == "transformer" and a.layout == "diffusers018":
        p.error("the diffusers 0.18 layout names attention processors only")
    from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict
    from regional_lora_ref import synthetic_adapter
    sd = random_state_dict(TINY_XL_CONFIG if a.config == "xl" else TINY_SD_CONFIG, seed=a.unet_seed)
    extra = ()
    if a.targets == "transformer":
        extra = [k[:-7] for k in sd if k.endswith(".weight") and ".attentions." in k and k[:-7].endswith((".ff.net.0.proj", ".ff.net.2", ".proj_in", ".proj_out"))]
    ck, truth = synthetic_adapter(sd, rank=a.rank, alpha=a.alpha, seed=a.seed, layout=a.layout, gain=a.gain, extra=extra)
    ck = {k: v.contiguous() for k, v in ck.items()}
    if a.out.endswith(".safetensors"):
        from safetensors.torch import save_file
        save_file(ck, a.out)
    else:
        import torch
        torch.save(ck, a.out)
    print(f"{a.out}: {len(truth)} adapted modules, rank {a.rank}, layout {a.layout}, {len(ck)} tensors")


if __name__ == "__main__":
    main()
