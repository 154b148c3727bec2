"""The optional paths of the UNet forward switched ON, bit for bit: tests/golden/engine_on_bits.json holds what tests/engine_golden.py's
on_digests() gave on an MI355X with the library of the parent of the commit that gave the UNet and the ControlNet one encoder walk and
split transformer() - the controlled forwards and three of their trace points, three controlled region steps, ControlNet + image prompts
+ regional LoRA together under the LayerNorm fold, every token map of a 12-step plain pass, the host-computed profile counters of a region
step and of the all-three forward, and the arena size of every engine built.  This tree reproduces all of it."""
import json

import pytest

pytestmark = pytest.mark.gpu

import engine_golden as G  # noqa: E402


def test_on_is_on_against_the_bits_of_the_commit_before():
    with open(G.BITS_JSON) as f:
        want = json.load(f)["digests"]
    got = G.on_digests()
    assert sorted(got) == sorted(want)
    differing = [k for k in want if got[k] != want[k]]
    for k in differing:
        print(f"{k}: got {got[k]}, recorded {want[k]}")
    assert not differing, differing
