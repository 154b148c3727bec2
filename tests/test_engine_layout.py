"""The engine's layout without a GPU: the ORDERED weight table, trace modules and attention modules of every (configuration, options)
pair equal tests/golden/engine_layout.json, recorded by tests/engine_golden.py on the parent of the commit that gave the UNet and the
ControlNet one encoder plan.  The order of the weight table is the order of the arena's allocations: a plan builder that registers a
slot earlier or later moves every weight behind it."""
import pytest

import engine_golden as G

PARENT, GOLDEN = G.load_layouts()

# the parent's own figures, as the issue that asked for this fixture quotes them: (weight slots, trace modules)
SANITY = {"tiny_xl/none": (620, 34), "tiny_xl/controlnet": (944, 61), "tiny_xl/all": (1386, 61),
          "sdxl/none": (1680, 34), "sdxl/controlnet": (2524, 61), "sdxl/all": (4344, 61)}


def _count(v):
    return v if isinstance(v, int) else len(v)


def test_the_fixture_is_the_parents():
    assert sorted(GOLDEN) == sorted(G.layout_keys())
    assert len(PARENT) == 40
    for key, (nw, nt) in SANITY.items():
        assert (_count(GOLDEN[key]["weights"]), _count(GOLDEN[key]["trace"])) == (nw, nt), key


@pytest.mark.parametrize("key", G.layout_keys())
def test_layout_is_the_recorded_one(key):
    got, want = G.layout_entry(*key.split("/")), GOLDEN[key]
    assert got == want, G.first_difference(got, want)
