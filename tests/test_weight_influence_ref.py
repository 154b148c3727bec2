"""The condition of tests/test_weight_influence_gpu.py, on the CPU with the oracle alone: EVERY 1-D tensor of both tiny state dicts (356 of
TINY_XL_CONFIG, 404 of TINY_SD_CONFIG) gets a perturbation that moves the output of the module that owns it by rho >= 0.1 (rel-L2) - so
that an engine which drops, doubles, negates or swaps the tensor cannot stay inside the GPU test's bound.  tests/weight_influence_ref.py
holds the rules (owner, ladder, prompt scale) and what had to be extended.  Also pinned here: the list of traceable modules is the same
in the oracle (ctl["trace"]), in the helper (from the config) and in the engine's plan (rt_trace_module_info, which needs no device),
with the same shapes.

Oracle time, 16 threads: about 0.25 s per full tiny forward, 60 s for all of tiny XL and 85 s for all of tiny SD, at most about 20 s per
case."""
import pytest
import torch

from oracle.unet import SD15_CONFIG, SDXL_CONFIG, TINY_SD_CONFIG, TINY_XL_CONFIG, OracleUNet, random_state_dict
import weight_influence_ref as W

CASES = {"tiny_xl": (TINY_XL_CONFIG, 16, 16, 356), "tiny_sd": (TINY_SD_CONFIG, 16, 32, 404)}
_state = {}


def influence(which):
    if which not in _state:
        cfg, h, w, _ = CASES[which]
        sd = random_state_dict(cfg, seed=11)
        _state[which] = W.Influence(cfg, sd, W.inputs(cfg, h, w))
    return _state[which]


PARAMS = [(which, g) for which, c in CASES.items() for g in W.groups(c[0])]


@pytest.mark.parametrize("which", list(CASES))
def test_groups_cover_every_one_d_tensor_once(which):
    cfg, _, _, n1d = CASES[which]
    inf = influence(which)
    tens = W.one_d_tensors(inf.sd)
    assert len(tens) == n1d
    gs = W.groups(cfg)
    assert len(set(gs)) == len(gs)
    by_group = {g: [k for _, k in tens if W.group_of(k) == g] for g in gs}
    assert sum(len(v) for v in by_group.values()) == n1d and all(by_group.values()), {g: len(v) for g, v in by_group.items()}
    for _, k in tens:
        assert W.owner(k, inf.modules) in inf.modules


@pytest.mark.parametrize("which,group", PARAMS, ids=[f"{a}-{b}" for a, b in PARAMS])
def test_every_one_d_tensor_moves_its_owner(which, group):
    inf = influence(which)
    rows = [inf.choose(i, k) for i, k in W.one_d_tensors(inf.sd) if W.group_of(k) == group]
    assert rows
    for r in rows:
        print(f"{which} {r['name']:<75s} @ {r['owner']:<28s} A {r['A']:.1f} prompt x{r['scale']:.0f} rho {r['rho']:.3f}")
    short = [(r["name"], r["rho"]) for r in rows if not r["rho"] >= W.RHO_MIN]
    assert not short, short
    assert all(r["A"] <= 2.0 or W.ladder(r["name"]) != W.LADDER for r in rows)
    assert all(torch.isfinite(r["d_ref"]).all() for r in rows)


def test_fold_width_tensors_move_their_owner():
    """The SDXL-width slice of the LayerNorm-fold case (weight_influence_ref.FOLD_CONFIG): its 24 tensors meet the same condition.
    About 25 s of oracle time (0.3 - 0.6 s per forward that ends at the observed transformer)."""
    sd = random_state_dict(W.FOLD_CONFIG, seed=11)
    inf = W.Influence(W.FOLD_CONFIG, sd, W.inputs(W.FOLD_CONFIG, *W.FOLD_LATENT), stop=W.FOLD_OWNERS[-1])
    tens = W.fold_tensors(sd)
    assert len(tens) == 24
    for i, k in tens:
        r = inf.choose(i, k)
        print(f"fold {r['name']:<75s} @ {r['owner']:<28s} A {r['A']:.1f} prompt x{r['scale']:.0f} rho {r['rho']:.3f}")
        assert r["rho"] >= W.RHO_MIN and torch.isfinite(r["d_ref"]).all(), (k, r["rho"])


@pytest.mark.parametrize("cfg,h,w", [(TINY_XL_CONFIG, 16, 24), (TINY_SD_CONFIG, 16, 32), (SDXL_CONFIG, 8, 8), (SD15_CONFIG, 8, 16)],
                         ids=["tiny_xl", "tiny_sd", "sdxl", "sd15"])
def test_traceable_modules_agree_between_oracle_helper_and_engine_plan(cfg, h, w):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(cfg, 64, 64, device=-1)          # weight-table-only engine: no GPU needed
    plan = e.trace_modules()
    e.close()
    names = W.trace_modules(cfg)
    assert [n for n, _, _ in plan] == names
    if cfg in (SDXL_CONFIG, SD15_CONFIG):
        return                                   # (the full-size weights are not drawn for a shape check: the tiny twins share the topology)
    tr = {}
    inp = W.inputs(cfg, h, w)
    o = OracleUNet(cfg, random_state_dict(cfg, seed=1))
    with torch.no_grad(), W.oracle_threads():
        out = o.forward(inp["lat"], W.T, inp["emb"], {"text_embeds": inp["pooled"], "time_ids": inp["tid"]} if inp["xl"] else None, ctl={"trace": tr})
    assert list(tr) == names and torch.equal(tr["conv_out"], out)
    for n, c, s in plan:
        assert tuple(tr[n].shape) == (1, c, h >> s, w >> s), (n, tuple(tr[n].shape), c, s)
    # trace_stop ends the forward behind the module and returns its tensor
    stop = names[len(names) // 2]
    tr2 = {}
    with torch.no_grad(), W.oracle_threads():
        got = o.forward(inp["lat"], W.T, inp["emb"], {"text_embeds": inp["pooled"], "time_ids": inp["tid"]} if inp["xl"] else None,
                        ctl={"trace": tr2, "trace_stop": stop})
    assert list(tr2) == names[:names.index(stop) + 1] and torch.equal(got, tr[stop])
