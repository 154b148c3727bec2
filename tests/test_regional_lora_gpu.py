"""Regional LoRA on the GPU (csrc/lora.hip, rt_op_lora_add): the op against the fp64 restatement of tests/regional_lora_ref.py at its
bar (the accumulation allowance twice the CPU emulation's), inside guarded / poisoned windows, bit-equal on a second launch, batch
invariant, with the streams that are not adapted keeping every byte; and what the launcher refuses."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import regional_lora_ref as R  # noqa: E402
from memguard import damage, guarded, intact, poisoned  # noqa: E402

DEV = "cuda:0"
LOG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "regional_lora_gpu_tests.log")


_logged = []


def _log(line):
    """Prints the figure and keeps it in profiles/regional_lora_gpu_tests.log (rewritten by every run of this module)."""
    print(line)
    _logged.append(line)
    try:
        with open(LOG, "w") as f:
            f.write("\n".join(_logged) + "\n")
    except OSError:
        pass


def _launch(inp, form, streams=None, pad=8):
    """The op on the inputs of regional_lora_ref.op_inputs, every operand in a guarded / poisoned window with leading dimensions `pad`
    larger than the packed widths.  streams: the subset of batch entries to launch (default all).  -> (Y after [B', rows, N] on the CPU,
    launched entries, (big, window) of Y for the guard check)."""
    from rich_text_to_image_amd.engine import lora_add
    X, Y = inp["X"], inp["Y"]
    streams = list(range(X.shape[0])) if streams is None else streams
    B, rows, K, N = len(streams), X.shape[1], X.shape[2], Y.shape[2]
    xd = poisoned(X[streams].reshape(B * rows, K).to(DEV), K + pad)
    dd, ud = poisoned(inp["down"].to(DEV), K + pad), poisoned(inp["up"].to(DEV), inp["up"].shape[1] + pad)
    ad, cd = poisoned(inp["aor"].to(DEV)), poisoned(inp["col"].to(DEV))
    y2 = Y[streams].reshape(B * rows, N)
    if form == "bf16_t":
        big, yd = guarded((N, B * rows), Y.dtype, B * rows + pad, fill="bytes", device=DEV)
        yd.copy_(y2.t())
    else:
        big, yd = guarded((B * rows, N), Y.dtype, N + pad, fill="bytes", device=DEV)
        yd.copy_(y2)
    n = lora_add(xd, dd, ud, ad, cd, yd, form, [b * rows for b in range(B)], [inp["scales"][s] for s in streams], rows)
    got = (yd.t() if form == "bf16_t" else yd).cpu().reshape(B, rows, N)
    return got, n, (big, yd)


def _bits(t):
    return t.contiguous().view(torch.int16)


@pytest.mark.parametrize("case", R.OP_CASES, ids=R.CASE_IDS)
def test_op_matches_the_fp64_restatement(case):
    """Every element of every adapted stream within the bar of Y + (f (X A^T)) B^T in fp64; the streams with all-zero scales keep every
    byte and are not in the grid; the guards and padding columns of Y stay intact and the poisoned surroundings of every input are never
    read (the result is finite); a second launch on the same inputs gives the same bits; head-pad columns keep their bits."""
    inp = R.op_inputs(case)
    form = case["form"]
    got, n, (big, yd) = _launch(inp, form)
    ref, bar = R.op_ref(inp, form, acc_units=R.GPU_ACC_UNITS)
    worst, share = R.worst_and_share(got, ref, bar)
    far, _ = R.worst_and_share(inp["Y"], ref, bar)
    _log(f"lora_add {case['name']} ({form}; streams {len(case['scales'])}, rows {case['rows']}, K {case['K']}, N {case['N']}, ranks {case['ranks']}): "
         f"worst |got - ref| / bar = {worst:.3f}; the input itself (no term) is at {far:.1f}")
    adapted = [b for b, s in enumerate(inp["scales"]) if any(s)]
    assert n == len(adapted)
    assert intact(big, yd), damage(big, yd)
    assert bool(torch.isfinite(got.float()).all())
    assert worst <= 1.0, share
    assert far > 50.0, far
    for b in range(len(inp["scales"])):
        if b not in adapted:
            assert torch.equal(_bits(got[b]), _bits(inp["Y"][b])), b
    if bool(inp["pad_rows"].any()):
        assert torch.equal(_bits(got[:, :, inp["pad_rows"]]), _bits(inp["Y"][:, :, inp["pad_rows"]]))
    again, _, _ = _launch(inp, form)
    assert torch.equal(_bits(again), _bits(got))


@pytest.mark.parametrize("case", [R.OP_CASES[1], R.OP_CASES[4], R.OP_CASES[5]], ids=[R.CASE_IDS[1], R.CASE_IDS[4], R.CASE_IDS[5]])
def test_op_is_batch_invariant(case):
    """An adapted stream launched alone, at row offset 0, equals the same stream inside the full launch, bit for bit."""
    inp = R.op_inputs(case)
    full, _, _ = _launch(inp, case["form"])
    for b, s in enumerate(inp["scales"]):
        if any(s):
            one, n, _ = _launch(inp, case["form"], streams=[b], pad=24)
            assert n == 1 and torch.equal(_bits(one[0]), _bits(full[b])), b


def test_op_launches_nothing_without_an_adapted_stream():
    inp = R.op_inputs(R.OP_CASES[0])
    inp["scales"] = [[0.0] * 4]
    got, n, (big, yd) = _launch(inp, "bf16")
    assert n == 0 and torch.equal(_bits(got), _bits(inp["Y"])) and intact(big, yd)


def test_op_refuses_what_it_cannot_do():
    from rich_text_to_image_amd.engine import RtError, lora_add
    inp = R.op_inputs(R.OP_CASES[0])

    def call(rows=8, R_=16, scales=((1.0,),), rows_at=(0,), form="bf16"):
        X, Y = inp["X"][0].to(DEV), inp["Y"][0].to(DEV)
        down, up = torch.zeros(R_, 32, dtype=torch.bfloat16, device=DEV), torch.zeros(16, R_, dtype=torch.bfloat16, device=DEV)
        return lora_add(X, down, up, torch.zeros(R_, device=DEV), torch.zeros(R_, dtype=torch.int32, device=DEV), Y, form, list(rows_at), list(scales), rows)
    assert call() == 1
    for kw in (dict(R_=8), dict(R_=144), dict(rows=4), dict(scales=((float("nan"),),)), dict(scales=((float("inf"),),)), dict(rows_at=(0,) * 17, scales=((1.0,),) * 17)):
        with pytest.raises(RtError) as e:
            call(**kw)
        assert e.value.code == -1, kw


# ---------------------------------------------------------------------------------------------------------------- the engine
import functools  # noqa: E402
import json  # noqa: E402

from freeu_ref import FORWARD_BAR, forward_case, rel_l2  # noqa: E402
from oracle.region_loop import rich_step_forwards  # noqa: E402
from oracle.unet import INJECT_RESNET, OracleUNet  # noqa: E402

STEP_BAR = 3e-2                  # latent UPDATE of one step against the composition of oracle forwards (tests/test_ip_adapter_gpu.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regional_lora_off_bits.json")
# adapter A: rank 4 (kohya, alpha 2) -> 16 rank columns, B: rank 8 (peft) -> 16: the engines below are built with lora_rank = 32
# prompt slots [negative, region 0, region 1, base] -> scales of (A, B): negative none, region 0 B at 1.0, region 1 both, base A at 0.7
SLOT_SCALES = ((0.0, 0.0), (0.0, 1.0), (0.5, 0.8), (0.7, 0.0))


def _engine(cfg, h, w, sd, **kw):
    from rich_text_to_image_amd.engine import Engine
    e = Engine(cfg, h, w, device=0, **kw)
    e.load_state_dict(sd)
    assert e.weights_missing()[0] == 0
    return e


@functools.lru_cache(maxsize=None)
def _adapters(which):
    """Two synthetic adapters for the tiny config's UNet: (state dict, [checkpoint A, checkpoint B], {name: modules})."""
    from rich_text_to_image_amd.regional_lora import parse_adapter
    from oracle.unet import TINY_SD_CONFIG, TINY_XL_CONFIG, random_state_dict
    cfg = TINY_XL_CONFIG if which == "xl" else TINY_SD_CONFIG
    sd = random_state_dict(cfg, seed=11)
    ckA, _ = R.synthetic_adapter(sd, rank=4, alpha=2.0, seed=1, layout="kohya", gain=2.0)
    ckB, _ = R.synthetic_adapter(sd, rank=8, seed=2, layout="peft", gain=1.0)
    return sd, [ckA, ckB], {"A": parse_adapter(sd, ckA)[0], "B": parse_adapter(sd, ckB)[0]}


def _lora_case(which):
    """forward_case with a fourth prompt: slots [negative, region 0, region 1, base]."""
    c = dict(forward_case(which))
    g = torch.Generator().manual_seed(99)
    c["emb"] = torch.cat([c["emb"][:2], torch.randn(1, 77, c["cfg"]["cross_attention_dim"], generator=g), c["emb"][2:]])
    if c["xl"]:
        c["pooled"] = torch.cat([c["pooled"][:2], torch.randn(1, 32, generator=g), c["pooled"][2:]])
    return c


def _set_prompts(eng, c):
    if c["xl"]:
        eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
    else:
        eng.set_prompts(c["emb"].to(DEV))


# streams: uncond (slot 0), base (3), text_ref (3, the reference latents), region (1), region (2), injected region (1, attends and injects from text_ref)
PROMPTS, QK_SRC, RES_SRC = [0, 3, 3, 1, 2, 1], [0, 1, 2, 3, 4, 2], [-1, -1, -1, -1, -1, 2]


def _forward(eng, c):
    lats = [c["lat"], c["lat"], c["lat_ref"], c["lat"], c["lat"], c["lat"]]
    x = torch.cat(lats).to(DEV)
    return eng.unet_forward(x, c["t"], PROMPTS, qk_src=QK_SRC, res_src=RES_SRC).cpu()


def _oracle_forward(c, sd, cks, slot_scales):
    def added(k):
        return {"text_embeds": c["pooled"][k:k + 1], "time_ids": c["tid"]} if c["xl"] else None
    o = R.lora_oracle(c["cfg"], sd, cks, [slot_scales[p] for p in PROMPTS])
    emb, t, out = c["emb"], c["t"], []
    with torch.no_grad():
        for k, p in enumerate(PROMPTS):
            lat = c["lat_ref"] if k == 2 else c["lat"]
            if k == 2:
                cap = {}
                out.append(o.forward(lat, t, emb[p:p + 1], added(p), ctl={"capture": cap})[0])
                inj = {n: v for n, v in cap.items() if n.endswith("attn1") or n == INJECT_RESNET}
            elif k == 5:
                out.append(o.forward(lat, t, emb[p:p + 1], added(p), ctl={"inject": inj})[0])
            else:
                out.append(o.forward(lat, t, emb[p:p + 1], added(p))[0])
    return out


@pytest.mark.parametrize("which", ["sd", "xl"])
def test_forward_with_stream_modes_matches_the_merged_oracle(which):
    """One batched forward of six streams - uncond at scale 0, base with adapter A at 0.7, text_ref likewise, a region with B at 1.0, a
    region with both, an injected region with B - against the CPU oracle run, per stream, with that stream's MERGED weights
    (lora.merge_lora per adapter at the stream's scales), at the project's forward bar.  The adapted streams are at least 5 bars from
    the un-adapted forward; the scale-0 stream equals it bit for bit.  Clearing the scales restores the un-adapted bits and the attn2
    caches that set_prompts left."""
    sd, cks, adapters = _adapters(which)
    c = _lora_case(which)
    eng = _engine(c["cfg"], c["h"], c["w"], sd, lora_rank=32)
    try:
        assert eng.bind_regional_loras(adapters) == ["A", "B"]
        _set_prompts(eng, c)
        caches0 = [(k.clone(), v.clone()) for k, v in eng.attn_caches()]
        plain = _forward(eng, c)
        eng.set_lora_scales(SLOT_SCALES)
        assert any(not torch.equal(k, k0) for (k, _), (k0, _) in zip(eng.attn_caches(), caches0))
        got = _forward(eng, c)
        ref = _oracle_forward(c, sd, cks, SLOT_SCALES)
        for k, name in enumerate(("uncond", "base A 0.7", "text_ref A 0.7", "region B 1.0", "region A 0.5 + B 0.8", "injected region B 1.0")):
            r, d = rel_l2(got[k], ref[k]), rel_l2(got[k], plain[k])
            _log(f"forward {which} stream {name}: rel-L2 vs merged oracle {r:.3e}; vs the un-adapted forward {d:.3e}")
            assert r < FORWARD_BAR, name
            if k == 0:
                assert torch.equal(got[0], plain[0])
            else:
                assert d >= 5 * FORWARD_BAR, name
        eng.set_lora_scales([(0.0, 0.0)] * 4)
        assert all(torch.equal(k, k0) and torch.equal(v, v0) for (k, v), (k0, v0) in zip(eng.attn_caches(), caches0))
        assert torch.equal(_forward(eng, c), plain)
    finally:
        eng.close()


def test_isolation_and_slot_permutation():
    """An adapted stream alone, next to other adapted streams and on an engine built for more prompts gives the same bits; permuting the
    prompt slots together with their scales changes nothing."""
    sd, cks, adapters = _adapters("xl")
    c = _lora_case("xl")
    eng = _engine(c["cfg"], c["h"], c["w"], sd, lora_rank=32)
    big = _engine(c["cfg"], c["h"], c["w"], sd, lora_rank=32, max_prompts=12)
    try:
        outs = []
        for e in (eng, big):
            e.bind_regional_loras(adapters)
            _set_prompts(e, c)
            e.set_lora_scales(SLOT_SCALES)
            outs.append(_forward(e, c))
        assert torch.equal(outs[0], outs[1])
        for k in (1, 3, 4):
            alone = eng.unet_forward(c["lat"].to(DEV), c["t"], [PROMPTS[k]]).cpu()
            assert torch.equal(alone[0], outs[0][k]), k
        perm = [3, 2, 0, 1]                                          # new slot i holds old slot perm[i]
        inv = [perm.index(p) for p in range(4)]
        c2 = dict(c); c2["emb"] = c["emb"][perm]; c2["pooled"] = c["pooled"][perm]
        _set_prompts(eng, c2)
        eng.set_lora_scales([SLOT_SCALES[p] for p in perm])
        x = torch.cat([c["lat"], c["lat"], c["lat_ref"], c["lat"], c["lat"], c["lat"]]).to(DEV)
        got = eng.unet_forward(x, c["t"], [inv[p] for p in PROMPTS], qk_src=QK_SRC, res_src=RES_SRC).cpu()
        assert torch.equal(got, outs[0])
    finally:
        eng.close(); big.close()


def test_off_is_off_against_the_bits_of_the_commit_before():
    """tests/golden/regional_lora_off_bits.json holds the sha256 of the tiny forwards and of one region step, recorded on the GPU by
    controlnet_ref.off_digests on the commit before regional LoRA existed.  This tree reproduces them with lora_rank = 0, with adapters
    loaded and every scale 0, and with scales set and then cleared."""
    from controlnet_ref import off_digests
    with open(GOLDEN) as f:
        want = json.load(f)["digests"]

    def with_adapters(cfg, h, w, sd):
        from rich_text_to_image_amd.regional_lora import parse_adapter
        e = _engine(cfg, h, w, sd, lora_rank=32)
        ck, _ = R.synthetic_adapter(sd, rank=4, alpha=2.0, seed=1, gain=2.0)
        e.bind_regional_loras({"A": parse_adapter(sd, ck)[0]})
        return e

    def set_and_clear(eng, c):
        P = c["emb"].shape[0]
        eng.set_lora_scales([(0.9,)] * P)
        eng.set_lora_scales([(0.0,)] * P)
    assert off_digests(lambda cfg, h, w, sd: _engine(cfg, h, w, sd)) == want
    assert off_digests(with_adapters) == want
    assert off_digests(with_adapters, lambda eng, c: eng.set_lora_scales([(0.0,)] * c["emb"].shape[0])) == want
    assert off_digests(with_adapters, set_and_clear) == want


# ---------------------------------------------------------------------------------------------------------------- steps
STEP_GS = 2.0


def _rich_case():
    """controlnet_ref.rich_case with two adapters and guidance scale STEP_GS.  (At that request's own guidance scale 5 the error of the
    step WITHOUT adapters - the parent's code: off is off, bit for bit - against the un-adapted oracle measures 2.91e-2 / 2.98e-2 on the
    latent update, main / reference stream, and 2.86e-2 / 3.08e-2 with the adapters on: the request leaves no headroom under the 3e-2
    bar with or without them.  The error of eps_u + g (eps_t - eps_u) grows with g for the same per-forward error, so the adapter step
    tests run the request at g = 2; the bar stays.)"""
    from controlnet_ref import rich_case
    c = dict(rich_case())
    c["gs"] = STEP_GS
    from rich_text_to_image_amd.regional_lora import parse_adapter
    ckA, _ = R.synthetic_adapter(c["sd"], rank=4, alpha=2.0, seed=1, layout="kohya", gain=2.0)
    ckB, _ = R.synthetic_adapter(c["sd"], rank=8, seed=2, layout="diffusers", gain=1.0)
    c["cks"], c["adapters"] = [ckA, ckB], {"A": parse_adapter(c["sd"], ckA)[0], "B": parse_adapter(c["sd"], ckB)[0]}
    return c


def _rich_reset(eng, c):
    eng.set_schedule(0, c["sched"].timesteps.tolist(), c["sched"].sigmas.tolist(), c["steps"])
    eng.set_latents(c["lat"].to(DEV))


@pytest.fixture(scope="module")
def rich():
    c = _rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd"], lora_rank=32)
    eng.bind_regional_loras(c["adapters"])
    eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
    eng.set_masks(c["masks"].to(DEV))
    eng.set_fontsize(torch.tensor([3, 5]), torch.tensor([4.0, -2.0]))
    eng.set_lora_scales(SLOT_SCALES)
    yield c, eng
    eng.close()


def test_region_step_matches_the_composition_of_merged_oracle_forwards(rich):
    """The injected first region_step (7 streams: uncond, base, uncond_ref, text_ref, three regions) with the base on adapter A, region 0
    on B and region 1 on both: both latent streams after the scheduler step against rich_step_forwards on the oracle with each forward's
    merged weights, on the latent UPDATE."""
    c, eng = rich
    R_ = c["masks"].shape[0]
    _rich_reset(eng, c)
    eng.region_step(0, c["gs"], c["isa"], 0.0, xl=True)
    got, got_ref = (t.cpu() for t in eng.read_latents(c["hw"], c["hw"], with_ref=True))
    sched, lat0, gs = c["sched"], c["lat"], c["gs"]
    t = sched.timesteps[0]
    slots = [0, R_, 0, R_] + list(range(1, R_))                      # the forwards of rich_step_forwards, by prompt slot

    def added_fn(k):
        k = k if k >= 0 else c["pooled"].shape[0] + k
        return {"text_embeds": c["pooled"][k:k + 1], "time_ids": c["tid"]}
    lat_in = sched.scale_model_input(lat0, t)
    tfd = {"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])}
    masks = [c["masks"][r:r + 1] for r in range(R_)]

    def compose(unet):
        eu, et, eur, etr = rich_step_forwards(unet, lat_in, lat_in.clone(), t, c["emb"], added_fn, masks, tfd, True, True)
        out = sched.step(torch.cat([eu + gs * (et - eu), eur + gs * (etr - eur)]), t, torch.cat([lat0, lat0]))["prev_sample"]
        return torch.chunk(out, 2, dim=0)
    ref, ref_ref = compose(R.lora_oracle(c["cfg"], c["sd"], c["cks"], [SLOT_SCALES[s] for s in slots]))
    pl, pl_ref = compose(OracleUNet(c["cfg"], c["sd"]))
    r, rr = rel_l2(got - lat0, ref - lat0), rel_l2(got_ref - lat0, ref_ref - lat0)
    d, dr = rel_l2(pl - lat0, ref - lat0), rel_l2(pl_ref - lat0, ref_ref - lat0)
    _log(f"region_step with regional LoRA: latent UPDATE rel-L2 {r:.3e} (reference stream {rr:.3e}); the un-adapted oracle is {d:.3e} / {dr:.3e} away")
    assert r < STEP_BAR and rr < STEP_BAR
    assert d > 3 * STEP_BAR and dr > 3 * STEP_BAR


def test_plain_step_matches_the_composition_of_merged_oracle_forwards():
    """plain_step (streams [uncond = slot 0, text = slot 1]) with adapter A at 0.7 and B at 0.4 on the text prompt only."""
    c = _rich_case()
    eng = _engine(c["cfg"], c["hw"], c["hw"], c["sd"], lora_rank=32)
    sc = [(0.0, 0.0), (0.7, 0.4)]
    try:
        eng.bind_regional_loras(c["adapters"])
        emb, pooled = c["emb"][[0, 3]], c["pooled"][[0, 3]]
        eng.set_prompts(emb.to(DEV), pooled.to(DEV), c["tid"])
        eng.set_lora_scales(sc)
        _rich_reset(eng, c)
        eng.plain_step(0, c["gs"])
        got = eng.read_latents(c["hw"], c["hw"]).cpu()
    finally:
        eng.close()
    sched, lat0, gs = c["sched"], c["lat"], c["gs"]
    t = sched.timesteps[0]
    x = sched.scale_model_input(lat0, t)

    def compose(unet):
        with torch.no_grad():
            eu = unet.forward(x, t, emb[:1], {"text_embeds": pooled[:1], "time_ids": c["tid"]})
            et = unet.forward(x, t, emb[1:], {"text_embeds": pooled[1:], "time_ids": c["tid"]})
        return sched.step(eu + gs * (et - eu), t, lat0)["prev_sample"]
    ref = compose(R.lora_oracle(c["cfg"], c["sd"], c["cks"], sc))
    pl = compose(OracleUNet(c["cfg"], c["sd"]))
    r, d = rel_l2(got - lat0, ref - lat0), rel_l2(pl - lat0, ref - lat0)
    _log(f"plain_step with regional LoRA: latent UPDATE rel-L2 {r:.3e}; the un-adapted oracle is {d:.3e} away")
    assert r < STEP_BAR
    assert d > 3 * STEP_BAR


def test_split_step_equals_the_whole_step_with_adapters(rich):
    """rt_region_step_part for both parts of two, then _finish, gives the bits of rt_region_step."""
    c, eng = rich
    for i in (0, c["steps"] - 1):
        _rich_reset(eng, c)
        eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=True)
        whole = eng.read_latents(c["hw"], c["hw"], with_ref=True)
        _rich_reset(eng, c)
        ranges = [eng.region_step_part(i, c["gs"], c["isa"], c["ibg"], True, part, 2)[:2] for part in (0, 1)]
        assert all(n > 0 for _, n in ranges), ranges
        eng.region_step_finish(i, c["gs"], c["isa"], c["ibg"], True)
        parts = eng.read_latents(c["hw"], c["hw"], with_ref=True)
        assert torch.equal(parts[0], whole[0]) and torch.equal(parts[1], whole[1]), i


def test_region_step_with_adapters_is_hipgraph_capturable(rich):
    """Nothing is allocated and nothing synchronises inside the step (rows and scales travel in the kernel arguments): the replay of a
    captured step gives the eager step's bits."""
    c, eng = rich
    hw = c["hw"]
    _rich_reset(eng, c)
    eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
    eager = eng.read_latents(hw, hw).clone()
    side = torch.cuda.Stream()
    eng.synchronize()
    eng.set_stream(side.cuda_stream)
    try:
        _rich_reset(eng, c)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=side):
            eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
        for _ in range(2):
            _rich_reset(eng, c)
            torch.cuda.synchronize()
            graph.replay()
            torch.cuda.synchronize()
            assert torch.equal(eng.read_latents(hw, hw), eager)
    finally:
        torch.cuda.synchronize()
        eng.set_stream(None)
    _rich_reset(eng, c)


def test_folded_layer_at_the_sdxl_block_shape():
    """weight_influence_ref.FOLD_CONFIG - levels of 640 and 1280 channels at SDXL's head dim, one transformer block each, on the 40 x 32
    latent at which every consumer of the blocks' LayerNorms takes the folded form: the adapters read a LayerNorm computed for the
    adapted rows only, and the partials a producing GEMM emitted are recomputed for those rows.  Three streams (scale 0, A, A + B)
    against the merged oracle; the scale-0 stream keeps its bits and an adapted stream alone gives its bits in the batch."""
    from oracle.unet import random_state_dict
    from rich_text_to_image_amd.regional_lora import parse_adapter
    from weight_influence_ref import FOLD_CONFIG, FOLD_LATENT
    cfg, (h, w) = FOLD_CONFIG, FOLD_LATENT
    sd = random_state_dict(cfg, seed=4)
    ckA, _ = R.synthetic_adapter(sd, rank=4, alpha=2.0, seed=1, gain=2.0)
    ckB, _ = R.synthetic_adapter(sd, rank=8, seed=2, layout="peft")
    g = torch.Generator().manual_seed(8)
    emb = torch.randn(3, 77, cfg["cross_attention_dim"], generator=g)
    lat = torch.randn(1, 4, h, w, generator=g)
    sc = [(0.0, 0.0), (0.7, 0.0), (0.5, 0.8)]
    eng = _engine(cfg, h, w, sd, lora_rank=32, max_streams=4, max_prompts=4)
    try:
        eng.bind_regional_loras({"A": parse_adapter(sd, ckA)[0], "B": parse_adapter(sd, ckB)[0]})
        eng.set_prompts(emb.to(DEV))
        x = torch.cat([lat] * 3).to(DEV)
        plain = eng.unet_forward(x, 500.0, [0, 1, 2]).cpu()
        eng.set_lora_scales(sc)
        got = eng.unet_forward(x, 500.0, [0, 1, 2]).cpu()
        alone = eng.unet_forward(lat.to(DEV), 500.0, [2]).cpu()
    finally:
        eng.close()
    o = R.lora_oracle(cfg, sd, [ckA, ckB], sc)
    with torch.no_grad():
        ref = [o.forward(lat, 500.0, emb[k:k + 1])[0] for k in range(3)]
    assert torch.equal(got[0], plain[0]) and torch.equal(alone[0], got[2])
    for k in range(3):
        r, d = rel_l2(got[k], ref[k]), rel_l2(got[k], plain[k])
        _log(f"folded 640 / 1280-wide blocks, stream {k} scales {sc[k]}: rel-L2 vs merged oracle {r:.3e}; vs the un-adapted forward {d:.3e}")
        assert r < FORWARD_BAR, k
        assert k == 0 or d >= 5 * FORWARD_BAR, k


def test_adapters_are_profiled_under_their_own_class(rich):
    c, eng = rich
    import ctypes as C
    _rich_reset(eng, c)
    eng.profile_enable(True)
    eng.region_step(0, c["gs"], c["isa"], c["ibg"], xl=True)
    eng.synchronize()
    n, ms, fl, by = C.c_int(), C.c_double(), C.c_double(), C.c_double()
    assert eng.lib.rt_profile_read2(eng.h, 9, C.byref(n), C.byref(ms), C.byref(fl), C.byref(by)) == 0
    eng.profile_enable(False)
    blocks = eng.lib.rt_attn_module_count(eng.h) // 2
    assert n.value == 6 * blocks and fl.value > 0 and by.value > 0 and ms.value > 0, (n.value, blocks)


def test_refusals_leave_the_engine_usable(rich):
    """RT_E_INVALID for a non-finite scale, more slots than prompts, NULL scales, a column map of the wrong length or while scales are set,
    and every call on an engine without adapters; the state is unchanged: the next forward keeps its bits."""
    import ctypes as C
    from rich_text_to_image_amd.engine import RtError
    c, eng = rich
    x = c["lat"].to(DEV)
    before = eng.unet_forward(x, 500.0, [3]).cpu()
    for bad in ([(0.0, float("nan"))] * 4, [(float("inf"),)] * 4, list(SLOT_SCALES) + [(1.0,)], []):
        with pytest.raises(RtError) as e:
            eng.set_lora_scales(bad)
        assert e.value.code == -1, bad
        assert torch.equal(eng.unet_forward(x, 500.0, [3]).cpu(), before)
    assert eng.lib.rt_set_lora_scales(eng.h, None, 4) == -1
    assert eng.lib.rt_set_lora_columns(eng.h, (C.c_int * 16)(), 16) == -1
    assert eng.lib.rt_set_lora_columns(eng.h, (C.c_int * 32)(), 32) == -1            # scales are set
    assert torch.equal(eng.unet_forward(x, 500.0, [3]).cpu(), before)
    off = _engine(c["cfg"], c["hw"], c["hw"], c["sd"])
    try:
        off.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
        with pytest.raises(RtError):
            off.set_lora_scales(SLOT_SCALES)
        with pytest.raises(RtError):
            off.bind_regional_loras(c["adapters"])
    finally:
        off.close()


# ---------------------------------------------------------------------------------------------------------------- facade
def _facade(c, sd=None):
    from rich_text_to_image_amd.region_diffusion_sdxl import RegionDiffusionXL
    m = RegionDiffusionXL(device=0, unet_state_dict=sd or c["sd"], config=c["cfg"])
    m.masks = [c["masks"][r:r + 1] for r in range(c["masks"].shape[0])]
    return m


def test_facade_matches_the_merged_pipeline_and_the_engine_loop():
    """tiny XL, 3 steps.  load_regional_loras + set_lora_scales(scale=s) - every slot, the negative prompt included - against the same
    pipeline built on the weights lora.merge_lora gives at scale s (what lora_path=, lora_scale=s loads): the latent update after 3 steps
    within the step bar, rich and plain pass.  A per-region request equals a hand-driven engine loop with that slot matrix bit for bit;
    a region index beyond the request's regions raises before any launch; clear_lora_scales() and unload_regional_loras() restore the
    bits of a pipeline that never loaded an adapter."""
    from rich_text_to_image_amd.lora import merge_lora
    c = _rich_case()
    hw, n, s = c["hw"], 3, 0.7
    tfd = {"word_pos": torch.tensor([3, 5]), "font_size": torch.tensor([4.0, -2.0])}
    lat_in = c["lat"].clone() / c["sched"].init_noise_sigma

    def sample(m, rich=True):
        return m.sample(prompt=None, height=8 * hw, width=8 * hw, num_inference_steps=n, guidance_scale=c["gs"], latents=lat_in.clone(),
                        prompt_embeds=c["emb"][1:] if rich else c["emb"][-1:], negative_prompt_embeds=c["emb"][:1],
                        pooled_prompt_embeds=c["pooled"][1:] if rich else c["pooled"][-1:], negative_pooled_prompt_embeds=c["pooled"][:1],
                        output_type="latent", run_rich_text=rich, text_format_dict=tfd, inject_selfattn=c["isa"], inject_background=c["ibg"]).images.cpu()
    never, never_plain = sample(_facade(c)), sample(_facade(c), rich=False)
    m = _facade(c)
    rep = m.load_regional_loras({"A": c["cks"][0]})
    assert sorted(rep["A"]["applied"]) == sorted(R.attention_projections(c["sd"])) and rep["A"]["dropped"] == []
    assert torch.equal(sample(m), never)                                         # adapters without a request: off is off
    m.set_lora_scales(scale=s)
    merged = _facade(c, merge_lora(c["sd"], c["cks"][0], s)[0])
    for rich, base in ((True, never), (False, never_plain)):
        got, want = sample(m, rich), sample(merged, rich)
        # on the latent UPDATE of the three steps; the run without adapters must itself be outside the bar, or a pipeline that ignored
        # the adapters would pass
        r, d = rel_l2(got - c["lat"], want - c["lat"]), rel_l2(base - c["lat"], want - c["lat"])
        _log(f"facade {'rich' if rich else 'plain'} pass, 3 steps, scale {s} on every slot vs the merged pipeline: latent UPDATE rel-L2 {r:.3e}; "
             f"the pipeline without adapters is {d:.3e} away")
        assert r < STEP_BAR and d > STEP_BAR
    # two adapters, a per-region request, by hand
    m.load_regional_loras({"A": c["cks"][0], "B": c["cks"][1]})
    m.set_lora_scales(scale={"A": 0.7}, regions={0: {"B": 1.0}, 1: {"A": 0.5, "B": 0.8}}, negative=0.0)
    on = sample(m)
    eng = _engine(c["cfg"], hw, hw, c["sd"], lora_rank=32)
    try:
        eng.bind_regional_loras(c["adapters"])
        eng.set_prompts(c["emb"].to(DEV), c["pooled"].to(DEV), c["tid"])
        eng.set_lora_scales(SLOT_SCALES)
        eng.set_masks(c["masks"].to(DEV))
        eng.set_fontsize(tfd["word_pos"], tfd["font_size"])
        m.scheduler.set_timesteps(n)
        eng.set_schedule(m.scheduler.kind, m.scheduler.timesteps.tolist(), m.scheduler.table(), n)
        eng.set_latents(lat_in.to(DEV).float() * m.scheduler.init_noise_sigma)
        for i in range(n):
            eng.region_step(i, c["gs"], c["isa"], c["ibg"], xl=True)
        assert torch.equal(eng.read_latents(hw, hw).cpu(), on)
    finally:
        eng.close()
    with pytest.raises(ValueError, match="region 2"):                            # a request with two region prompts
        m.set_lora_scales(regions={2: {"A": 0.5}})
        sample(m)
    with pytest.raises(ValueError, match="2 adapters are loaded"):
        m.set_lora_scales(scale=0.5)
    m.clear_lora_scales()
    assert torch.equal(sample(m), never)
    m.unload_regional_loras()
    assert torch.equal(sample(m), never) and m.regional_loras is None


def test_sample_cli_round_trip(tmp_path):
    """python -m rich_text_to_image_amd.sample --region_lora A.safetensors:0:0.9 B.pt:base:0.6 on a synthetic tiny-SD checkpoint and two
    adapters written by tools/make_regional_lora.py (kohya and peft layouts): both files are read from disk; the rich pass - where region 0
    exists - and the plain pass - whose base prompt carries B - differ from the run without them; a "region_loras" key of a --requests
    line sets the scales of that request alone."""
    import json
    import sys
    from rich_text_to_image_amd import sample
    from test_checkpoint_gpu import _write_dir
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import make_regional_lora
    _write_dir(str(tmp_path / "ckpt"))
    a, b = str(tmp_path / "watercolour.safetensors"), str(tmp_path / "pixel.pt")
    make_regional_lora.main([a, "--config", "sd", "--rank", "4", "--alpha", "2", "--layout", "kohya", "--seed", "1"])
    make_regional_lora.main([b, "--config", "sd", "--rank", "8", "--layout", "peft", "--seed", "2", "--gain", "1"])
    js = json.dumps({"ops": [{"insert": "a "}, {"attributes": {"link": "a wooden fence covered in snow"}, "insert": "fence"},
                             {"insert": " under a night sky\n"}]})
    common = ["--load_path", str(tmp_path / "ckpt"), "--model", "SD", "--sample_steps", "12", "--seed", "3", "--num_segments", "4", "--inject_selfattn", "0.2"]
    plain0, rich0 = sample.main(common + ["--rich_text_json", js, "--run_dir", str(tmp_path / "out0")])
    plain, rich = sample.main(common + ["--rich_text_json", js, "--run_dir", str(tmp_path / "out"), "--region_lora", f"{a}:0:0.9", f"{b}:base:0.6"])
    assert plain.shape == rich.shape == (1, 512, 512, 3)
    assert os.path.exists(tmp_path / "out" / "seed3_plain.jpg") and os.path.exists(tmp_path / "out" / "seed3_rich.jpg")
    assert (plain != plain0).any() and (rich != rich0).any()
    with open(tmp_path / "reqs.jsonl", "w") as f:
        f.write(json.dumps({"rich_text_json": json.loads(js), "seed": 3, "region_loras": [f"{a}:0:0.9", f"{b}:base:0.6"]}) + "\n")
        f.write(json.dumps({"rich_text_json": json.loads(js), "seed": 3}) + "\n")
    out = sample.main(common + ["--requests", str(tmp_path / "reqs.jsonl"), "--run_dir", str(tmp_path / "out2")])
    assert out is not None
    with pytest.raises(SystemExit, match="file not found"):
        sample.main(common + ["--rich_text_json", js, "--region_lora", str(tmp_path / "missing.safetensors")])
    with pytest.raises(SystemExit, match="TARGET"):
        sample.main(common + ["--rich_text_json", js, "--region_lora", f"{a}:sky"])
