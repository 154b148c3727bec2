"""TEST INFRASTRUCTURE: generate tests/golden/reference_unet.pt from the UNMODIFIED reference UNet2DConditionModel.

Runs only where the reference tree is present (oracle/refload.py).  Stores what tests/test_oracle_vs_reference.py pins the oracle
against, so that the test runs on any checkout:
  * the reference's state_dict layout (name -> shape) at the tiny, SD-v1.5 and SDXL-base configurations (full sizes built on the meta
    device), and
  * for the two tiny configurations, one batch-2 forward at t = 481 of the reference module with oracle.unet.random_state_dict(seed=1)
    loaded, together with its inputs.
Usage:  python -m oracle.make_reference_unet_golden
"""
import os

import torch

from .refload import load_reference
from .unet import SD15_CONFIG, SDXL_CONFIG, TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict, reference_kwargs

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "reference_unet.pt")


def main():
    U = load_reference()["unet_2d_condition"].UNet2DConditionModel
    out = {"layout": {}, "forward": {}}
    for name, cfg in (("sd15", SD15_CONFIG), ("sdxl", SDXL_CONFIG)):
        with torch.device("meta"):
            m = U(**reference_kwargs(cfg))
        out["layout"][name] = {k: tuple(v.shape) for k, v in m.state_dict().items()}
    for name, cfg, xl in (("tiny_xl", TINY_XL_CONFIG, True), ("tiny_sd", TINY_SD_CONFIG, False)):
        m = U(**reference_kwargs(cfg))
        out["layout"][name] = {k: tuple(v.shape) for k, v in m.state_dict().items()}
        m.load_state_dict(random_state_dict(cfg, seed=1))
        torch.manual_seed(0)
        B = 2
        x, ctx = torch.randn(B, 4, 32, 32), torch.randn(B, 77, cfg["cross_attention_dim"])
        added = {"text_embeds": torch.randn(B, 32), "time_ids": torch.tensor([[32., 32, 0, 0, 32, 32]] * B)} if xl else None
        with torch.no_grad():
            y = m(x, torch.tensor(481), encoder_hidden_states=ctx, added_cond_kwargs=added)["sample"]
        out["forward"][name] = {"x": x, "t": 481, "ctx": ctx, "added": added, "reference_sample": y}
    torch.save(out, OUT)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
